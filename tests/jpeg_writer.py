"""A test-side writer of baseline / extended-sequential Huffman JPEG files, written from ITU-T T.81 (Annexes B, C, F and K.2).

It exists to make VALID files that no libjpeg encoder writes: any Huffman table shape, any table ids, several scans with their own
tables and restart intervals, 16-bit quantization tables, any component ids and sampling factors, coefficients of any amplitude a
Huffman symbol exists for, stray markers and fill bytes.  It is a pure function from a description to bytes (numpy only):

    data, stats = write_jpeg(width, height, comps, coefs, qtables, scans, sof=0, header="jfif", extras=None)

    comps    [(component id, h, v, quantization table number), ...] in frame order
    coefs    per component an int array [block rows][block cols][64 zig-zag], padded to whole MCUs (padded_blocks()); the blocks
             beyond real_blocks() are coded in interleaved scans only, as the format demands
    qtables  {table number: (precision 0 = 8-bit / 1 = 16-bit, 64 steps in zig-zag order)}
    scans    [dict(comps=[frame indices, ascending], dc=[table id per component], ac=[...], ri=restart interval in MCUs (0: none),
             shape=one of SHAPES or (DC shape, AC shape)), ...]; every scan gets a DHT segment of its own in front of it that
             defines the tables it names from the symbols it uses, and a DRI segment whenever its interval is not the one in force
    sof      0 (SOF0) or 1 (SOF1)
    header   "jfif", ("adobe", transform 0 / 1 / 2) or None
    extras   dict of hooks: after_soi / before_scan (lists of raw segments, e.g. TEM, COM(b"..."), APPN(5, b"...")), fill (fill
             bytes 0xFF in front of {"DHT", "SOS", "EOI", "DQT", "SOF", "DRI"} markers), tail (bytes behind EOI)

stats: long_share (share of code words longer than 8 bits), codes, and per scan its tables {("dc" | "ac", id): (bits, huffval)}.

No table holds the all-ones code word (T.81 C.2 / K.2 reserve it); entropy-coded data is byte-stuffed, every restart segment is
padded with 1-bits, RSTn counts modulo 8."""
import heapq

import numpy as np

SHAPES = ("optimal", "all16", "deep", "all9", "full256")
TEM = b"\xff\x01"


def COM(text):
    return b"\xff\xfe" + (len(text) + 2).to_bytes(2, "big") + bytes(text)


def APPN(n, payload):
    return bytes([0xFF, 0xE0 + n]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def _ceil(a, b):
    return -(-a // b)


def frame_mcus(width, height, comps):
    maxh, maxv = max(c[1] for c in comps), max(c[2] for c in comps)
    return _ceil(width, 8 * maxh), _ceil(height, 8 * maxv)


def padded_blocks(width, height, comps, ci):
    """(block rows, block columns) of component ci padded to whole MCUs: the shape of its coefficient array"""
    mx, my = frame_mcus(width, height, comps)
    return my * comps[ci][2], mx * comps[ci][1]


def real_blocks(width, height, comps, ci):
    """(block rows, block columns) that hold samples of the image (T.81 A.1.1): ceil(ceil(X * h / hmax) / 8)"""
    maxh, maxv = max(c[1] for c in comps), max(c[2] for c in comps)
    return _ceil(_ceil(height * comps[ci][2], maxv), 8), _ceil(_ceil(width * comps[ci][1], maxh), 8)


# ---- Huffman tables: code lengths per shape, then the canonical codes of Annex C ---------------------------------------------------
def _optimal_lengths(freq):
    """K.2: Huffman code lengths of the symbols with freq > 0 plus one reserved symbol (it takes the all-ones code word and is dropped
    from the table), then the length limit of Figure K.3.  Returns {symbol: length}."""
    syms = [s for s in range(256) if freq[s] > 0]
    heap = [(int(freq[s]), s, (s,)) for s in syms] + [(0, 256, (256,))]
    heapq.heapify(heap)
    length = dict.fromkeys(syms + [256], 0)
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        for s in a[2] + b[2]:
            length[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    bits = [0] * 40
    for s in length:
        bits[max(length[s], 1)] += 1
    i = 39
    while i > 16:                                          # Figure K.3 (Adjust_BITS)
        if bits[i] == 0:
            i -= 1
            continue
        j = i - 2
        while bits[j] == 0:
            j -= 1
        bits[i] -= 2
        bits[i - 1] += 1
        bits[j + 1] += 2
        bits[j] -= 1
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                           # the reserved symbol leaves from the longest length
    order = sorted(syms, key=lambda s: (length[s], s))     # shorter codes to the symbols the tree gave shorter codes
    out, k = {}, 0
    for l in range(1, 17):
        for _ in range(bits[l]):
            out[order[k]] = l
            k += 1
    assert k == len(syms)
    return out


def make_table(freq, shape, dc):
    """(bits[17], huffval list) of a table of `shape` for the symbols with freq > 0:
    optimal  frequency-optimal, limited to 16 bits          all16 / all9  every code 16 / 9 bits long
    deep     lengths 1..7 for seven symbols, 16 for the rest    full256  all 256 symbols (AC only), the unused ones behind the used"""
    syms = sorted((s for s in range(256) if freq[s] > 0), key=lambda s: (-int(freq[s]), s))
    if not syms:
        syms = [0]
    if shape == "full256" and dc:
        shape = "optimal"                                  # a DC table holds categories only
    if shape == "all16":
        length = {s: 16 for s in syms}
    elif shape == "all9":
        length = {s: 9 for s in syms}
    elif shape == "deep":
        syms = syms[::-1]                                  # the short codes go to the seven RAREST symbols: most code words are long
        length = {s: (i + 1 if i < 7 else 16) for i, s in enumerate(syms)}
    elif shape == "full256":
        syms = syms + [s for s in range(256) if s not in set(syms)]
        length = {s: (8 if i < 254 else 9) for i, s in enumerate(syms)}
    elif shape == "optimal":
        f = np.zeros(256, np.int64)
        f[syms] = [max(int(freq[s]), 1) for s in syms]
        length = _optimal_lengths(f)
    else:
        raise ValueError("table shape %r" % (shape,))
    order = sorted(syms, key=lambda s: (length[s], syms.index(s)))
    bits = [0] * 17
    for s in order:
        bits[length[s]] += 1
    return bits, order


def canonical_codes(bits, huffval):
    """Annex C: (code[256], size[256]) of a table; size 0 = no code.  Asserts that the all-ones code word of no length is used."""
    code, size = np.zeros(256, np.int64), np.zeros(256, np.int64)
    c, k = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l]):
            assert c < (1 << l) - 1, "the all-ones code word of %d bits" % l
            code[huffval[k]], size[huffval[k]] = c, l
            c += 1
            k += 1
        c <<= 1
    return code, size


# ---- one scan: symbols, tables, bits ---------------------------------------------------------------------------------------------
def _scan_blocks(width, height, comps, coefs, scan_comps):
    """the blocks of a scan in coding order: (coefficients [n][64], component-in-scan [n], MCU number [n])"""
    if len(scan_comps) == 1:
        ci = scan_comps[0]
        rows, cols = real_blocks(width, height, comps, ci)
        a = np.asarray(coefs[ci])[:rows, :cols].reshape(-1, 64)
        return a.astype(np.int64), np.zeros(len(a), np.int64), np.arange(len(a), dtype=np.int64)
    mx, my = frame_mcus(width, height, comps)
    parts, js = [], []
    for j, ci in enumerate(scan_comps):
        h, v = comps[ci][1], comps[ci][2]
        a = np.asarray(coefs[ci])
        assert a.shape == (my * v, mx * h, 64), "component %d: %s, padded to whole MCUs it is %s" % (ci, a.shape, (my * v, mx * h, 64))
        parts.append(a.reshape(my, v, mx, h, 64).transpose(0, 2, 1, 3, 4).reshape(my * mx, v * h, 64))
        js += [j] * (v * h)
    blk = np.concatenate(parts, axis=1)                    # [MCU][block in MCU][64]
    bpm = blk.shape[1]
    assert bpm <= 10, "%d blocks in an MCU" % bpm
    return (blk.reshape(-1, 64).astype(np.int64), np.tile(np.array(js, np.int64), my * mx), np.repeat(np.arange(my * mx, dtype=np.int64), bpm))


def _category(v):
    a = np.abs(v)
    s = np.zeros(a.shape, np.int64)
    nz = a > 0
    s[nz] = np.floor(np.log2(a[nz])).astype(np.int64) + 1
    return s


def _scan_events(blk, jcomp, mcu, ri):
    """every code word of the scan in order: arrays (block, class 0 DC / 1 AC, symbol, extra bits, extra length)"""
    n = len(blk)
    seg = mcu // ri if ri else np.zeros(n, np.int64)
    dc = blk[:, 0]
    diff = np.zeros(n, np.int64)
    for j in np.unique(jcomp):
        idx = np.nonzero(jcomp == j)[0]
        d = dc[idx].copy()
        prev = np.concatenate([[0], d[:-1]])
        prev[np.concatenate([[True], seg[idx][1:] != seg[idx][:-1]])] = 0
        diff[idx] = d - prev
    s = _category(diff)
    assert s.max(initial=0) <= 15, "a DC difference no category exists for"
    ev = [(np.arange(n), np.zeros(n, np.int64), np.zeros(n, np.int64), s, np.where(diff < 0, diff + (1 << s) - 1, diff), s)]
    b, k = np.nonzero(blk[:, 1:])
    k = k + 1
    v = blk[b, k]
    first = np.concatenate([[True], b[1:] != b[:-1]]) if len(b) else np.zeros(0, bool)
    prevk = np.where(first, 0, np.concatenate([[0], k[:-1]])) if len(b) else k
    run = k - prevk - 1
    s = _category(v)
    assert s.max(initial=0) <= 15, "an AC value no category exists for"
    ev.append((b, k * 4 + 3, np.ones(len(b), np.int64), ((run & 15) << 4) | s, np.where(v < 0, v + (1 << s) - 1, v), s))
    for t in range(3):                                     # up to three ZRL symbols in front of a coefficient
        m = run // 16 > t
        ev.append((b[m], k[m] * 4 + t, np.ones(m.sum(), np.int64), np.full(m.sum(), 0xF0, np.int64), np.zeros(m.sum(), np.int64), np.zeros(m.sum(), np.int64)))
    last = np.zeros(n, np.int64)
    if len(b):
        np.maximum.at(last, b, k)
    e = np.nonzero(last < 63)[0]                           # EOB, unless the block ends on position 63
    ev.append((e, np.full(len(e), 64 * 4, np.int64), np.ones(len(e), np.int64), np.zeros(len(e), np.int64), np.zeros(len(e), np.int64), np.zeros(len(e), np.int64)))
    cols = [np.concatenate([x[i] for x in ev]) for i in range(6)]
    order = np.lexsort((cols[1], cols[0]))
    block, _, cls, sym, extra, elen = [c[order] for c in cols]
    return block, cls, sym, extra, elen, seg


def _pack(values, lengths):
    """bit fields (value, length <= 16), most significant bit first, to bytes; the total is a multiple of 8"""
    total = int(lengths.sum())
    assert total % 8 == 0
    start = np.cumsum(lengths) - lengths
    pos = np.arange(total, dtype=np.int64) - np.repeat(start, lengths)
    bits = (np.repeat(values, lengths) >> (np.repeat(lengths, lengths) - 1 - pos)) & 1
    return np.packbits(bits.astype(np.uint8)).tobytes()


def _write_scan(width, height, comps, coefs, scan):
    """(DHT payloads, entropy-coded bytes with RSTn markers, tables, code lengths of every code word)"""
    sc = scan["comps"]
    assert list(sc) == sorted(set(sc)), "scan components in frame order"
    shape = scan.get("shape", "optimal")
    dshape, ashape = (shape, shape) if isinstance(shape, str) else shape
    ri = int(scan.get("ri", 0))
    blk, jcomp, mcu = _scan_blocks(width, height, comps, coefs, sc)
    block, cls, sym, extra, elen, seg = _scan_events(blk, jcomp, mcu, ri)
    ids = np.where(cls == 0, np.array(scan["dc"], np.int64)[jcomp[block]], np.array(scan["ac"], np.int64)[jcomp[block]])
    slot = cls * 4 + ids
    hist = np.bincount(slot * 256 + sym, minlength=8 * 256).reshape(8, 256)
    tables, code, size = {}, np.zeros((8, 256), np.int64), np.zeros((8, 256), np.int64)
    dht = b""
    for c, name in ((0, "dc"), (1, "ac")):
        for t in sorted(set(scan[name])):
            assert 0 <= t <= 3
            bits, vals = make_table(hist[c * 4 + t], dshape if c == 0 else ashape, c == 0)
            tables[(name, t)] = (bits, vals)
            code[c * 4 + t], size[c * 4 + t] = canonical_codes(bits, vals)
            dht += bytes([c * 16 + t]) + bytes(bits[1:]) + bytes(vals)
    clen = size[slot, sym]
    assert (clen > 0).all()
    # code word and extra bits side by side, a field of 1-bits behind the last block of every restart segment
    ev_seg = seg[block]
    vals = np.stack([code[slot, sym], extra], axis=1).reshape(-1)
    lens = np.stack([clen, elen], axis=1).reshape(-1)
    nseg = int(seg.max()) + 1
    seg_bits = np.bincount(ev_seg, weights=clen + elen, minlength=nseg).astype(np.int64)
    pad = (-seg_bits) % 8
    ends = np.cumsum(np.bincount(ev_seg, minlength=nseg)) * 2          # index behind every segment's last field
    vals = np.insert(vals, ends, (1 << pad) - 1)
    lens = np.insert(lens, ends, pad)
    raw = _pack(vals, lens)
    cut = np.concatenate([[0], np.cumsum((seg_bits + pad) // 8)])
    out = bytearray()
    for k in range(nseg):
        if k:
            out += bytes([0xFF, 0xD0 + ((k - 1) & 7)])
        out += raw[cut[k]:cut[k + 1]].replace(b"\xff", b"\xff\x00")
    return dht, bytes(out), tables, clen


def _seg(marker, payload, fill=0):
    return b"\xff" * fill + bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def write_jpeg(width, height, comps, coefs, qtables, scans, sof=0, header="jfif", extras=None):
    x = dict(extras or {})
    fill = x.get("fill", {})
    out = bytearray(b"\xff\xd8")
    if header == "jfif":
        out += _seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    elif header is not None:
        assert header[0] == "adobe"
        out += _seg(0xEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, header[1]]))
    for raw in x.get("after_soi", []):
        out += raw
    for t in sorted(qtables):
        prec, q = qtables[t]
        q = [int(v) for v in q]
        assert len(q) == 64 and min(q) >= 1 and max(q) <= (65535 if prec else 255)
        out += _seg(0xDB, bytes([prec * 16 + t]) + (b"".join(v.to_bytes(2, "big") for v in q) if prec else bytes(q)), fill.get("DQT", 0))
    frame = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([len(comps)])
    for cid, h, v, tq in comps:
        frame += bytes([cid, h * 16 + v, tq])
    out += _seg(0xC0 + sof, frame, fill.get("SOF", 0))
    stats = dict(scans=[], codes=0, long=0)
    ri_in_force = 0
    for scan in scans:
        dht, data, tables, clen = _write_scan(width, height, comps, coefs, scan)
        for raw in x.get("before_scan", []):
            out += raw
        ri = int(scan.get("ri", 0))
        if ri != ri_in_force:
            out += _seg(0xDD, ri.to_bytes(2, "big"), fill.get("DRI", 0))
            ri_in_force = ri
        out += _seg(0xC4, dht, fill.get("DHT", 0))
        sos = bytes([len(scan["comps"])])
        for j, ci in enumerate(scan["comps"]):
            sos += bytes([comps[ci][0], scan["dc"][j] * 16 + scan["ac"][j]])
        out += _seg(0xDA, sos + bytes([0, 63, 0]), fill.get("SOS", 0))
        out += data
        stats["scans"].append(tables)
        stats["codes"] += len(clen)
        stats["long"] += int((clen > 8).sum())
    out += b"\xff" * fill.get("EOI", 0) + b"\xff\xd9" + x.get("tail", b"")
    stats["long_share"] = stats["long"] / max(stats["codes"], 1)
    return bytes(out), stats
