"""A test-side writer of Huffman-coded progressive JPEG files (SOF2), written from ITU-T T.81 Annex G (G.1.2, Figures G.3 - G.7): the
progressive half of tests/jpeg_writer.py, whose tables (make_table, canonical_codes), bit packing, block order, byte stuffing, restart
padding, marker segments and `extras` hooks it uses as they are.  Like write_jpeg it exists to make VALID files that no libjpeg
encoder writes, and is a pure function from a description to bytes (numpy only): see write_progressive."""
import numpy as np

from jpeg_writer import _category, _pack, _scan_blocks, _seg, canonical_codes, make_table, padded_blocks, real_blocks


class _Fields:
    """the bit fields of a scan in order: a Huffman symbol of table slot (class * 4 + id) or raw bits (slot -1), with its restart segment"""
    def __init__(self):
        self.slot, self.val, self.len, self.seg = [], [], [], []

    def sym(self, seg, slot, s):
        self.slot.append(slot)
        self.val.append(s)
        self.len.append(0)
        self.seg.append(seg)

    def bits(self, seg, v, n):
        if n:
            self.slot.append(-1)
            self.val.append(v)
            self.len.append(n)
            self.seg.append(seg)

    def arrays(self):
        return tuple(np.array(x, np.int64) for x in (self.slot, self.val, self.len, self.seg))


def _dc_first(blk, jcomp, seg, al, slots):
    """G.1.2.1: the differences of the shifted DC values, coded as F.1.2.1 does"""
    n = len(blk)
    dc = blk[:, 0] >> al
    diff = np.zeros(n, np.int64)
    for j in np.unique(jcomp):
        idx = np.nonzero(jcomp == j)[0]
        d = dc[idx]
        prev = np.concatenate([[0], d[:-1]])
        prev[np.concatenate([[True], seg[idx][1:] != seg[idx][:-1]])] = 0
        diff[idx] = d - prev
    s = _category(diff)
    assert s.max(initial=0) <= 11, "a DC difference beyond 8-bit data"
    extra = np.where(diff < 0, diff + (1 << s) - 1, diff)
    slot = np.stack([np.asarray(slots, np.int64)[jcomp], np.full(n, -1, np.int64)], axis=1).reshape(-1)
    return slot, np.stack([s, extra], axis=1).reshape(-1), np.stack([np.zeros(n, np.int64), s], axis=1).reshape(-1), np.repeat(seg, 2)


def _split_run(n, policy, rng, turn):
    """the EOBn run lengths a maximal run of n blocks is written as"""
    if policy == "max":
        return [n]
    if policy == "none":
        return [1] * n
    out, left = [], n
    while left:
        kind = turn[0] % 6
        turn[0] += 1
        r = int(rng.integers(1, max(left.bit_length(), 2)))
        p = (1, 2, 3, 1 << r, (1 << r) - 1, int(rng.integers(1, left + 1)))[kind]
        p = max(1, min(p, left, n - 1 if n > 1 else 1))                    # a run of two or more blocks is always cut
        out.append(p)
        left -= p
    return out


def _ac_first_block(c, ss, se, al, extra_zrl):
    """Figure G.3 for one block -> (fields [(symbol or -1, bits, length)], an EOB is needed, no bits behind it)"""
    ev, r = [], 0
    for k in range(ss, se + 1):
        v = int(c[k])
        t = abs(v) >> al
        if t == 0:
            r += 1
            continue
        while r > 15:
            ev.append((0xF0, 0, 0))
            r -= 16
        s = t.bit_length()
        ev.append(((r << 4) | s, t if v > 0 else t ^ ((1 << s) - 1), s))
        r = 0
    if extra_zrl and r >= 17:
        ev.append((0xF0, 0, 0))
    return ev, r > 0, (0, 0)


def _ac_refine_block(c, ss, se, al, extra_zrl):
    """Figure G.7 for one block -> (fields, an EOB is needed, the correction bits behind it (value, count))"""
    ab = [abs(int(v)) >> al for v in c[ss:se + 1]]
    eobpos = max((k for k, t in enumerate(ab) if t == 1), default=-1)
    ev, r, bv, bn = [], 0, 0, 0
    for k, t in enumerate(ab):
        if t == 0:
            r += 1
            continue
        while r > 15 and k <= eobpos:
            ev.append((0xF0, bv, bn))
            r, bv, bn = r - 16, 0, 0
        if t > 1:
            bv, bn = (bv << 1) | (t & 1), bn + 1
            continue
        ev.append(((r << 4) | 1, (((1 if c[ss + k] > 0 else 0) << bn) | bv), bn + 1))
        r, bv, bn = 0, 0, 0
    if extra_zrl:
        # behind the last newly non-zero coefficient: the ZRL takes the bits in front of the 16th zero-history position, if any
        # position lies behind that one (the decoder then reads one more symbol for this block, the EOB)
        zeros, taken = 0, 0
        for k in range(eobpos + 1, len(ab)):
            if ab[k] == 0:
                zeros += 1
                if zeros == 16:
                    if k < len(ab) - 1:
                        ev.append((0xF0, bv >> (bn - taken), taken))
                        bv, bn, r = bv & ((1 << (bn - taken)) - 1), bn - taken, r - 16
                    break
            else:
                taken += 1
    return ev, r > 0 or bn > 0, (bv, bn)


def _ac_scan(blk, seg, scan, slot, st):
    """an AC scan's fields: the blocks' own symbols, and the EOB runs merged by the scan's policy"""
    ss, se, ah, al = scan["Ss"], scan["Se"], scan["Ah"], scan["Al"]
    policy = scan.get("eob", "max")
    rng = np.random.default_rng(policy[1]) if isinstance(policy, tuple) else None
    if isinstance(policy, tuple):
        assert policy[0] == "split"
        policy = "split"
    extra_zrl = scan.get("zrl", "needed") == "before_eob"
    assert scan.get("zrl", "needed") in ("needed", "before_eob") and policy in ("max", "none", "split")
    one = _ac_refine_block if ah else _ac_first_block
    a = np.abs(blk[:, ss:se + 1]) >> al
    busy = a.any(axis=1)
    if ah:
        st["max_correction"] = int((a > 1).sum(axis=1).max(initial=0))
    n = len(blk)
    empty = ([], True, (0, 0))
    rec = [one(blk[b], ss, se, al, extra_zrl) if busy[b] or (extra_zrl and se - ss >= 16) else empty for b in range(n)]
    F, turn, i = _Fields(), [0], 0
    while i < n:
        ev, needs, _ = rec[i]
        g = int(seg[i])
        for s, v, l in ev:
            F.sym(g, slot, s)
            F.bits(g, v, l)
            st["zrl"] += s == 0xF0
        if not needs:
            i += 1
            continue
        j = i + 1
        while j < n and j - i < 32767 and seg[j] == g and not rec[j][0] and rec[j][1]:
            j += 1
        for p in _split_run(j - i, policy, rng, turn):
            r = p.bit_length() - 1
            F.sym(g, slot, r << 4)
            F.bits(g, p - (1 << r), r)
            st["eob"][r] += 1
            st["eob_blocks"] += p
            for b in range(i, i + p):
                if rec[b][2][1]:
                    F.bits(g, *rec[b][2])
            i += p
    return F.arrays()


def _prog_fields(width, height, comps, coefs, scan, st):
    """(slot, value, length, segment) of every field of a scan, and its number of restart segments"""
    sc = list(scan["comps"])
    assert sc == sorted(set(sc)), "scan components in frame order"
    ss, se, ah, al = scan["Ss"], scan["Se"], scan["Ah"], scan["Al"]
    assert (ss == 0 and se == 0) or (1 <= ss <= se <= 63 and len(sc) == 1), "a scan is DC only, or AC of one component"
    assert 0 <= al <= 13 and (ah == 0 or ah == al + 1)
    ri = int(scan.get("ri", 0))
    blk, jcomp, mcu = _scan_blocks(width, height, comps, coefs, sc)
    seg = mcu // ri if ri else np.zeros(len(blk), np.int64)
    if ss:
        f = _ac_scan(blk, seg, scan, 4 + scan["ac"][0], st)
    elif ah == 0:
        f = _dc_first(blk, jcomp, seg, al, scan["dc"])
    else:                                                  # G.1.2.1: one bit a block
        n = len(blk)
        f = (np.full(n, -1, np.int64), (blk[:, 0] >> al) & 1, np.ones(n, np.int64), seg)
    return f, int(seg.max()) + 1


def _entropy_bytes(f, nseg, code, size, st):
    """the fields as bytes: code words looked up, every restart segment padded with 1-bits and byte-stuffed, RSTn between them"""
    slot, val, length, seg = f
    is_sym = slot >= 0
    s_, v_ = np.where(is_sym, slot, 0), np.where(is_sym, val, 0)
    clen = size[s_, v_]
    assert (clen[is_sym] > 0).all(), "a symbol without a code word"
    vals, lens = np.where(is_sym, code[s_, v_], val), np.where(is_sym, clen, length)
    st["codes"], st["long"] = int(is_sym.sum()), int((clen[is_sym] > 8).sum())
    seg_bits = np.bincount(seg, weights=lens, minlength=nseg).astype(np.int64)
    pad = (-seg_bits) % 8
    ends = np.cumsum(np.bincount(seg, minlength=nseg))
    assert (np.diff(seg) >= 0).all() and (np.bincount(seg, minlength=nseg) > 0).all()
    raw = _pack(np.insert(vals, ends, (1 << pad) - 1), np.insert(lens, ends, pad))
    cut = np.concatenate([[0], np.cumsum((seg_bits + pad) // 8)])
    out = bytearray()
    for k in range(nseg):
        if k:
            out += bytes([0xFF, 0xD0 + ((k - 1) & 7)])
        part = raw[cut[k]:cut[k + 1]]
        st["stuffed"] += part.count(b"\xff")
        out += part.replace(b"\xff", b"\xff\x00")
    return bytes(out)


def _table_set(scan, k):
    d = scan.get("dht", "own")
    if d == "own":
        return ("own", k)
    if d == "upfront":
        return ("upfront",)
    assert isinstance(d, tuple) and d[0] == "group", "dht: %r" % (d,)
    return d


def write_progressive(width, height, comps, coefs, qtables, scans, header="jfif", extras=None):
    """-> (bytes, stats, expected): a progressive file (SOF2); comps, coefs, qtables, header and extras as write_jpeg takes them

    scans    [dict(comps=[frame indices], Ss, Se, Ah, Al, dc=[table id per component], ac=[...], ri, shape, eob, zrl, dht, also), ...]
             eob   the EOB-run policy of an AC scan: "max" (runs up to 32767, ended by a restart boundary and the end of the scan),
                   "none" (EOB0 for every block that needs one) or ("split", seed): every maximal run cut at seeded points into
                   pieces of 1, 2, 3, 2^r and 2^r - 1 blocks.  In a refinement scan the correction bits of a run's blocks follow
                   the EOBn symbol that ends them (G.1.2.3), however many they are
             zrl   "needed" (default) or "before_eob": one extra ZRL in front of an EOB wherever sixteen zero (in a refinement:
                   zero-history) positions and one more position of the band lie behind the block's last coded coefficient, so that
                   the decoder still reads the EOB for this block
             dht   "own" (default): a DHT in front of the scan, from its own symbol counts; ("group", name): one set of tables from the
                   summed counts of the group's scans, in front of the first of them; "upfront": such a set in front of the first SOS
             also  [("dc" | "ac", id), ...]: tables the scan's DHT segment defines as well (for the scan's own symbols of that class)
    expected per component an array like coefs: what the scans leave behind -- the value where a position reaches Al = 0, the
             point-transformed value shifted back where it stops above, 0 where it is never sent
    stats    long_share, codes, and per scan (stats["scans"][k]): tables, eob (EOBn symbols by r), eob_blocks (the blocks they end), zrl,
             dht (a DHT segment precedes the scan), max_correction (the most correction bits one block consumes), stuffed (0xFF bytes of entropy-coded data), codes, long

    DC first scans shift right arithmetically by Al, AC scans divide by 2^Al toward zero (G.1.2.1); the restart interval counts the
    scan's own MCUs (one block in a one-component scan).  The script is checked as it is walked: Ah is the Al before it, first scans come
    first, and every table a scan codes with is the one in force at its SOS."""
    x = dict(extras or {})
    fill = x.get("fill", {})
    nc = len(comps)
    # ---- the fields of every scan, what it leaves behind, and the symbol counts of every set of tables
    al_map = [np.full(np.asarray(coefs[ci]).shape, -1, np.int64) for ci in range(nc)]
    plans, sets = [], {}
    for k, scan in enumerate(scans):
        st = dict(eob=[0] * 15, eob_blocks=0, zrl=0, max_correction=0, stuffed=0, codes=0, long=0)
        f, nseg = _prog_fields(width, height, comps, coefs, scan, st)
        for ci in scan["comps"]:
            rows, cols = real_blocks(width, height, comps, ci) if len(scan["comps"]) == 1 else padded_blocks(width, height, comps, ci)
            m = al_map[ci][:rows, :cols, scan["Ss"]:scan["Se"] + 1]
            rr, rc = real_blocks(width, height, comps, ci)     # (blocks of padding are in interleaved scans only, and in no result)
            assert (m[:rr, :rc] == (scan["Ah"] if scan["Ah"] else -1)).all(), "scan %d: Ah is not the Al before it, or a first scan comes second" % k
            assert scan["Ss"] == 0 or (al_map[ci][:rr, :rc, 0] >= 0).all(), "scan %d: AC before DC" % k
            m[...] = scan["Al"]
        hist = np.bincount(f[0][f[0] >= 0] * 256 + f[1][f[0] >= 0], minlength=8 * 256).reshape(8, 256)
        need = [("ac", scan["ac"][0])] if scan["Ss"] else [("dc", t) for t in sorted(set(scan["dc"]))] if scan["Ah"] == 0 else []
        key = _table_set(scan, k)
        shape = scan.get("shape", "optimal")
        ts = sets.setdefault(key, dict(first=k, hist=np.zeros((8, 256), np.int64), names=[], shape=(shape, shape) if isinstance(shape, str) else shape))
        for name, t in need + list(scan.get("also", [])):
            assert 0 <= t <= 3
            slot = (name == "ac") * 4 + t
            if (name, t) in need:
                ts["hist"][slot] += hist[slot]
            else:                                              # a table nothing codes with: the scan's symbols of that class
                ts["hist"][slot] += hist[(name == "ac") * 4:(name == "ac") * 4 + 4].sum(axis=0)
            if (name, t) not in ts["names"]:
                ts["names"].append((name, t))
        plans.append((f, nseg, st, need, key))
    for ts in sets.values():
        ts["tables"], ts["dht"] = {}, b""
        for name, t in sorted(ts["names"]):
            c = name == "ac"
            bits, vals = make_table(ts["hist"][c * 4 + t], ts["shape"][c], not c)
            ts["tables"][(name, t)] = (bits, vals)
            ts["dht"] += bytes([c * 16 + t]) + bytes(bits[1:]) + bytes(vals)
    expected = []
    for ci in range(nc):
        a, m = np.asarray(coefs[ci]).astype(np.int64), np.maximum(al_map[ci], 0)
        e = np.where(a < 0, -((-a >> m) << m), (a >> m) << m)
        e[..., 0] = (a[..., 0] >> m[..., 0]) << m[..., 0]
        expected.append(np.where(al_map[ci] < 0, 0, e))
    # ---- the file
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
    frame = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([nc])
    for cid, h, v, tq in comps:
        frame += bytes([cid, h * 16 + v, tq])
    out += _seg(0xC2, frame, fill.get("SOF", 0))
    stats = dict(scans=[], codes=0, long=0)
    in_force, ri_in_force = {}, 0
    code, size = np.zeros((8, 256), np.int64), np.zeros((8, 256), np.int64)

    def define(ts):
        out.extend(_seg(0xC4, ts["dht"], fill.get("DHT", 0)))
        for (name, t), tab in ts["tables"].items():
            in_force[(name, t)] = tab
            code[(name == "ac") * 4 + t], size[(name == "ac") * 4 + t] = canonical_codes(*tab)

    if ("upfront",) in sets:
        define(sets[("upfront",)])
    for k, scan in enumerate(scans):
        f, nseg, st, need, key = plans[k]
        for raw in x.get("before_scan", []):
            out += raw
        ri = int(scan.get("ri", 0))
        if ri != ri_in_force:
            out += _seg(0xDD, ri.to_bytes(2, "big"), fill.get("DRI", 0))
            ri_in_force = ri
        ts = sets[key]
        if ts["first"] == k and key != ("upfront",) and ts["dht"]:
            define(ts)
        for name_t in need:
            assert in_force.get(name_t) == ts["tables"][name_t], "scan %d: table %s was redefined since its set was written" % (k, name_t)
        sos = bytes([len(scan["comps"])])
        for j, ci in enumerate(scan["comps"]):
            sos += bytes([comps[ci][0], scan.get("dc", [0] * 4)[j] * 16 + scan.get("ac", [0] * 4)[j]])
        out += _seg(0xDA, sos + bytes([scan["Ss"], scan["Se"], scan["Ah"] * 16 + scan["Al"]]), fill.get("SOS", 0))
        out += _entropy_bytes(f, nseg, code, size, st)
        st["tables"] = {name_t: ts["tables"][name_t] for name_t in need}
        st["dht"] = ts["first"] == k and key != ("upfront",) and bool(ts["dht"])
        stats["scans"].append(st)
        stats["codes"] += st["codes"]
        stats["long"] += st["long"]
    out += b"\xff" * fill.get("EOI", 0) + b"\xff\xd9" + x.get("tail", b"")
    stats["long_share"] = stats["long"] / max(stats["codes"], 1)
    return bytes(out), stats, expected
