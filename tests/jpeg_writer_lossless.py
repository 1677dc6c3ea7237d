"""A test-side writer of lossless Huffman JPEG files (SOF3), written from ITU-T T.81 Annex H (the lossless mode of operation) and
B.2 (the marker segments), on the table and bit-packing helpers of jpeg_writer.py.

It exists to make files that a lossless decoder must read and that no libjpeg encoder writes: a table slot of its own for every
component of a scan, tables of any shape, tables defined once for several scans or all in one segment, a restart interval per scan,
fill bytes in front of any marker, any component ids, and "running values" that use all 16 bits whatever the frame's precision
says.  It is a pure function from a description to bytes (numpy only):

    data, expected, stats = write_lossless(precision, planes, scans, ids=None, header=None, fill=None)

    precision  8, 12 or 16 (P of the frame header)
    planes     per component an integer array [H][W] of running values 0..65535: what the decoder holds BEFORE the point transform
               is undone.  All arithmetic is modulo 2^16 (H.1.2.1), so values beyond 2^(P - Pt) are coded like any other
    scans      [dict(comps=[frame indices, ascending], psv=1..7, pt=point transform, rows=restart interval in rows (0: none; it may
               exceed H), tables=[DC table slot per component], shape=..., dht=..., tables_from=..., fill=..., before=[...]), ...]
               shape        "optimal", "all16", "all9", "deep" (jpeg_writer.make_table), "deep17" (deep, with all 17 categories
                            defined, used or not) or a literal (bits[17], huffval list); or {slot: one of these}
               dht          where the scan's tables are defined: "own" (one DHT segment per table in front of its SOS; the default),
                            "merged" (one DHT segment with all of them in front of its SOS), "upfront" (in front of the FIRST SOS,
                            a segment per table) or "upfront_merged" (in front of the first SOS, in ONE segment with the tables of
                            every other scan that says so)
               tables_from  the index of an earlier scan: this scan defines nothing and codes with that scan's tables of the same
                            slots, which are then made from the categories of both
               fill         {"RST" | "SOS" | "DHT" | "DRI": number of fill bytes 0xFF in front of every such marker of this scan}
               before       raw marker segments (jpeg_writer.COM, APPN) written in front of everything else of this scan
    ids        component ids of the frame header; default 1, 2, 3
    header     None, "jfif" or ("adobe", transform)
    fill       the default of every scan's `fill`, and "EOI"

A DRI segment is written whenever the interval in force is not the scan's, a DRI of 0 behind a nonzero one included.

The coding (H.1.2): the first sample of a restart interval is predicted by 2^(P - Pt - 1), the rest of the interval's first row from
the left, the first sample of every other row from above, every other sample by the scan's predictor on full-width integers; the
difference is taken modulo 2^16; its category SSSS is coded with the component's table and followed by SSSS bits as for a DC
difference (H.1.2.2), except that category 16 is the difference 32768 and has none.  Every segment is padded with 1-bits, 0xFF data
bytes are stuffed, RSTn counts modulo 8.

expected: the samples a decoder must produce, (value << Pt) truncated to the sample type -- the low 8 bits (uint8) at P = 8, the
low 16 bits (uint16) at 12 and 16 -- as [H][W] for one component and [H][W][3] for three.

stats: {"dri": every DRI value written, in order, "dht": [(index of the scan it stands in front of, [slots of the segment])],
"scans": per scan dict(tables={slot: (bits, huffval)}, categories={slot: histogram[17]}, long_share=share of code words longer than
8 bits, ff_bytes=0xFF data bytes (each stuffed), data_bytes=length of the entropy-coded data with stuffing and markers,
rst=[marker codes written], dri=interval in MCUs in force)}."""
import numpy as np

from jpeg_writer import _pack, _seg, canonical_codes, make_table

SHAPES = ("optimal", "all16", "all9", "deep", "deep17")


def predictions(x, precision, pt, psv, rows):
    """the prediction of every sample of a plane of running values (H.1.2.1, Table H.1), as full-width integers"""
    x = np.asarray(x).astype(np.int64)
    h = x.shape[0]
    a, b, c = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    a[:, 1:] = x[:, :-1]
    b[1:] = x[:-1]
    c[1:, 1:] = x[:-1, :-1]
    p = (a, b, c, a + b - c, a + ((b - c) >> 1), b + ((a - c) >> 1), (a + b) >> 1)[psv - 1].copy()
    p[1:, 0] = x[:-1, 0]
    first = (np.arange(h) % rows == 0) if rows else (np.arange(h) == 0)
    p[first] = a[first]
    p[first, 0] = 1 << (precision - pt - 1)
    return p


def differences(x, precision, pt, psv, rows):
    """modulo 2^16"""
    return (np.asarray(x).astype(np.int64) - predictions(x, precision, pt, psv, rows)) & 0xFFFF


def categories(d):
    """(SSSS, the appended bits, their number) of differences modulo 2^16 (Table H.2)"""
    v = np.where(d > 32768, d - 65536, d)
    s = np.searchsorted(1 << np.arange(17, dtype=np.int64), np.abs(v), side="right").astype(np.int64)
    n = np.where(s == 16, 0, s)
    return s, np.where(s == 16, 0, np.where(v < 0, v + (1 << n) - 1, v)), n


def _shape_of(scan, slot):
    shape = scan.get("shape", "optimal")
    return shape[slot] if isinstance(shape, dict) else shape


def _table(hist, shape):
    if not isinstance(shape, str):
        bits, vals = list(shape[0]), list(shape[1])
        assert len(bits) == 17 and sum(bits[1:]) == len(vals)
        return bits, vals
    assert shape in SHAPES, shape
    if shape == "deep17":
        hist = hist.copy()
        hist[:17] += 1
        shape = "deep"
    return make_table(hist, shape, True)


def write_lossless(precision, planes, scans, ids=None, header=None, fill=None):
    planes = [np.asarray(p).astype(np.int64) for p in planes]
    h, w = planes[0].shape
    nc = len(planes)
    assert precision in (8, 12, 16) and all(p.shape == (h, w) and p.min() >= 0 and p.max() <= 0xFFFF for p in planes)
    ids = list(ids) if ids is not None else [1, 2, 3][:nc]
    fill0 = dict(fill or {})
    # ---- 1. every scan's symbols
    work = []
    for scan in scans:
        comps, slots, rows = list(scan["comps"]), list(scan["tables"]), int(scan.get("rows", 0))
        assert comps == sorted(set(comps)) and len(slots) == len(comps) and all(0 <= t <= 3 for t in slots)
        assert 1 <= scan["psv"] <= 7 and 0 <= scan["pt"] < precision and 0 <= rows * w <= 0xFFFF
        d = np.stack([differences(planes[c], precision, scan["pt"], scan["psv"], rows) for c in comps], axis=-1)       # [H][W][component]
        s, extra, elen = categories(d)
        slot = np.broadcast_to(np.array(slots, np.int64), s.shape)
        hist = np.bincount((slot * 17 + s).ravel(), minlength=4 * 17).reshape(4, 17)
        work.append(dict(s=s, extra=extra, elen=elen, slot=slot, hist={t: hist[t].copy() for t in sorted(set(slots))}, rows=rows))
    # ---- 2. tables: a scan's own, or an earlier scan's made from both
    symbols = [dict((t, np.concatenate([wk["hist"][t], np.zeros(256 - 17, np.int64)])) for t in wk["hist"]) for wk in work]
    for k, scan in enumerate(scans):
        j = scan.get("tables_from")
        if j is not None:
            assert 0 <= j < k and scans[j].get("tables_from") is None
            for t in symbols[k]:
                symbols[j][t] = symbols[j][t] + symbols[k][t]
    tables = []
    for k, scan in enumerate(scans):
        j = scan.get("tables_from")
        tables.append(tables[j] if j is not None else {t: _table(symbols[k][t], _shape_of(scan, t)) for t in sorted(symbols[k])})
    # ---- 3. the file
    out = bytearray(b"\xff\xd8")
    if header == "jfif":
        out += _seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    elif header is not None:
        assert header[0] == "adobe"
        out += _seg(0xEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, header[1]]))
    frame = bytes([precision]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([nc])
    for c in range(nc):
        frame += bytes([ids[c], 0x11, 0])
    out += _seg(0xC3, frame)
    stats = dict(dri=[], dht=[], scans=[])

    def payload(k, t):
        bits, vals = tables[k][t]
        return bytes([t]) + bytes(bits[1:]) + bytes(vals)

    in_force = {}                                           # slot -> the table a decoder holds at this point of the file
    merged = [(k, t) for k, scan in enumerate(scans) if scan.get("dht") == "upfront_merged" for t in sorted(tables[k])]
    ri_in_force = 0
    for k, (scan, wk) in enumerate(zip(scans, work)):
        f = dict(fill0)
        f.update(scan.get("fill", {}))
        for raw in scan.get("before", []):
            out += raw
        if k == 0:
            for j, other in enumerate(scans):
                if other.get("dht") == "upfront":
                    assert other.get("tables_from") is None
                    for t in sorted(tables[j]):
                        assert t not in in_force, "two tables for slot %d in front of the first scan" % t
                        out += _seg(0xC4, payload(j, t), f.get("DHT", 0))
                        stats["dht"].append((0, [t]))
                        in_force[t] = tables[j][t]
            if merged:
                assert len(set(t for _, t in merged)) == len(merged), "two tables for one slot in front of the first scan"
                out += _seg(0xC4, b"".join(payload(j, t) for j, t in merged), f.get("DHT", 0))
                stats["dht"].append((0, [t for _, t in merged]))
                in_force.update({t: tables[j][t] for j, t in merged})
        where = scan.get("dht", "own")
        assert where in ("own", "merged", "upfront", "upfront_merged"), where
        if scan.get("tables_from") is None and where in ("own", "merged"):
            if where == "merged":
                out += _seg(0xC4, b"".join(payload(k, t) for t in sorted(tables[k])), f.get("DHT", 0))
                stats["dht"].append((k, sorted(tables[k])))
            else:
                for t in sorted(tables[k]):
                    out += _seg(0xC4, payload(k, t), f.get("DHT", 0))
                    stats["dht"].append((k, [t]))
            in_force.update(tables[k])
        for t in tables[k]:
            assert in_force.get(t) is tables[k][t], "scan %d: slot %d holds another table when its SOS is met" % (k, t)
        ri = wk["rows"] * w
        if ri != ri_in_force:
            out += _seg(0xDD, ri.to_bytes(2, "big"), f.get("DRI", 0))
            stats["dri"].append(ri)
            ri_in_force = ri
        sos = bytes([len(scan["comps"])])
        for j, c in enumerate(scan["comps"]):
            sos += bytes([ids[c], scan["tables"][j] << 4])
        out += _seg(0xDA, sos + bytes([scan["psv"], 0, scan["pt"]]), f.get("SOS", 0))
        # the entropy-coded segments: code word and appended bits side by side, a field of 1-bits behind every segment's last sample
        code, size = np.zeros((4, 17), np.int64), np.zeros((4, 17), np.int64)
        for t in tables[k]:
            cd, sz = canonical_codes(*tables[k][t])
            assert not sz[17:].any(), "a lossless table holds categories 0..16"
            code[t], size[t] = cd[:17], sz[:17]
        s, slot = wk["s"].ravel(), wk["slot"].ravel()
        clen = size[slot, s]
        assert (clen > 0).all(), "a category its table has no code for"
        elen = wk["elen"].ravel()
        rows = wk["rows"]
        per_seg = (rows if rows and rows < h else h) * w * len(scan["comps"])
        nseg = -(-len(s) // per_seg)
        seg = np.arange(len(s), dtype=np.int64) // per_seg
        vals = np.stack([code[slot, s], wk["extra"].ravel()], axis=1).reshape(-1)
        lens = np.stack([clen, elen], axis=1).reshape(-1)
        seg_bits = np.bincount(seg, weights=clen + elen, minlength=nseg).astype(np.int64)
        pad = (-seg_bits) % 8
        ends = np.cumsum(np.bincount(seg, minlength=nseg)) * 2
        raw = _pack(np.insert(vals, ends, (1 << pad) - 1), np.insert(lens, ends, pad))
        cut = np.concatenate([[0], np.cumsum((seg_bits + pad) // 8)])
        data, rst = bytearray(), []
        for i in range(nseg):
            if i:
                rst.append(0xD0 + ((i - 1) & 7))
                data += b"\xff" * f.get("RST", 0) + bytes([0xFF, rst[-1]])
            data += raw[cut[i]:cut[i + 1]].replace(b"\xff", b"\xff\x00")
        out += data
        stats["scans"].append(dict(tables=dict(tables[k]), categories={t: wk["hist"][t] for t in wk["hist"]}, long_share=float((clen > 8).mean()),
                                   ff_bytes=raw.count(b"\xff"), data_bytes=len(data), rst=rst, dri=ri))
    out += b"\xff" * fill0.get("EOI", 0) + b"\xff\xd9"
    # ---- 4. what a decoder returns
    pts = [0] * nc
    coded = [0] * nc
    for scan in scans:
        for c in scan["comps"]:
            pts[c] = scan["pt"]
            coded[c] += 1
    assert coded == [1] * nc, "every component in exactly one scan"
    dt, mask = (np.uint8, 0xFF) if precision == 8 else (np.uint16, 0xFFFF)
    expected = np.stack([((p << pt) & mask).astype(dt) for p, pt in zip(planes, pts)], axis=-1)
    return bytes(out), (expected[:, :, 0] if nc == 1 else expected), stats
