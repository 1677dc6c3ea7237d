"""The case list and helpers of the arithmetic-source tests (test_simt_arith_sources.py on the emulator, test_gpu_arith_sources.py on
the chip): arithmetic-coded files (SOF9, SOF10) through mozjpeg_amd.decode_coefficients, decode, decode_planes and recompress with
arithmetic_sources=True, i.e. MJH_SRC_ARITHMETIC in mjh_jpeg_probe_ex / mjh_encoder_set_sources and the kernel of
mjh_decode_arith.hip.

Every source is made at test time by the reference (cjpeg -arithmetic, refenc for scan scripts and conditioning, jpegtran
-arithmetic for the four-component file); every expected value comes from the reference at test time: coefficient arrays from
tests/native/coef_dump on oracle/_ref/libjpeg.so.62, pixels from djpeg (tj3Decompress8 for four components), files from jpegtran
-copy none.  Every comparison is exact equality; decode_cases.djpeg asserts that the reference reads the file without a warning.

As prog_source_cases notes, `cjpeg -restart 1` in the default profile writes one DRI for scans whose MCU counts differ and the
reference warns on its own file: the restart cases use -revert."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

import oracle_lib as O
import cmyk_cases as CK
import coef_cases as CC
import decode_cases as DC
import djpeg_cases as DJ
import fast_idct_cases as FI
import prog_source_cases as PC
import transcode_cases as TC


def have_tools():
    return CC.have_tools() and DC.have_tools() and os.path.exists(os.path.join(O.REF_DIR, "refenc"))


def _arith(args, img=None, script=None):
    """cjpeg ... -arithmetic (behind -revert, which resets the entropy coder with everything else)"""
    return TC.cjpeg(TC.testorig() if img is None else img, args + ["-arithmetic"], script=script)


def _refenc(**kw):
    return O.ref_encode(TC.testorig(), arithmetic=True, **kw)[0]


def renumbered(jpeg, table_map):
    """the file with the table numbers of its DAC and SOS segments changed (a pure byte edit: every statistics area starts alike)"""
    b = bytearray(jpeg)
    pos = 2
    while pos < len(b):
        assert b[pos] == 0xFF
        m = b[pos + 1]
        n = (b[pos + 2] << 8) | b[pos + 3]
        if m == 0xCC:
            for o in range(pos + 4, pos + 2 + n, 2):
                b[o] = (b[o] & 0x10) | table_map.get(b[o] & 15, b[o] & 15)
        if m == 0xDA:
            for i in range(b[pos + 4]):
                o = pos + 6 + 2 * i
                b[o] = (table_map.get(b[o] >> 4, b[o] >> 4) << 4) | table_map.get(b[o] & 15, b[o] & 15)
            return bytes(b)          # (sequential, one scan)
        pos += 2 + n
    raise AssertionError("no SOS")


def ycck_arith():
    """a YCCK 4:2:0 file of the reference's TurboJPEG library, re-coded to sequential arithmetic by the reference's jpegtran"""
    return O.ref_jpegtran(CK.source("tj_ycck420"), ["-copy", "all", "-revert", "-arithmetic"])


SIMPLE = ["-revert", "-progressive"]
# name -> (maker, needs progressive_sources)
SOURCES = {
    # both file types on 227 x 149
    "seq_420": (lambda: _arith(["-revert"]), False),
    "seq_444": (lambda: _arith(["-revert", "-sample", "1x1"]), False),
    "seq_2x1": (lambda: _arith(["-revert", "-sample", "2x1"]), False),
    "seq_gray": (lambda: _arith(["-revert", "-grayscale"]), False),
    "prog_default": (lambda: _arith([]), True),
    "prog_simple": (lambda: _arith(SIMPLE), True),
    "prog_script_a": (lambda: _arith(["-revert"], script=PC.SCRIPT_A), True),
    "prog_script_b": (lambda: _arith(["-revert"], script=PC.SCRIPT_B), True),
    # partial MCUs and degenerate sizes
    "seq_17x9_2x1": (lambda: _arith(["-revert", "-sample", "2x1"], O.synthetic_frame(17, 9, 5)), False),
    "prog_17x9_2x1": (lambda: _arith(SIMPLE + ["-sample", "2x1"], O.synthetic_frame(17, 9, 5)), True),
    "seq_8x8": (lambda: _arith(["-revert"], O.synthetic_frame(8, 8, 4)), False),
    "prog_8x8": (lambda: _arith(SIMPLE, O.synthetic_frame(8, 8, 4)), True),
    "seq_1x1": (lambda: _arith(["-revert"], O.synthetic_frame(1, 1, 3)), False),
    "prog_1x1": (lambda: _arith(SIMPLE, O.synthetic_frame(1, 1, 3)), True),
    # restarts
    "seq_restart_rows": (lambda: _arith(["-revert", "-restart", "1"]), False),
    "prog_restart_rows": (lambda: _arith(SIMPLE + ["-restart", "1"]), True),
    "seq_restart_3b": (lambda: _arith(["-revert", "-restart", "3B"]), False),
    "prog_restart_3b": (lambda: _arith(SIMPLE + ["-restart", "3B"]), True),
    # non-interleaved sequential (the golden case script_seq_arith_y_cbcr_restart1)
    "seq_y_cbcr_restart1": (lambda: _refenc(restart=1, scans=[((0,), 0, 63, 0, 0), ((1, 2), 0, 63, 0, 0)]), False),
    # conditioning other than L 0, U 1, K 5
    "seq_cond": (lambda: _refenc(revert=True, arith_cond=((1, 3, 9), (0, 2, 20))), False),
    "prog_cond": (lambda: _refenc(revert=True, progressive=True, arith_cond=((0, 15, 12), (3, 4, 2))), True),
    # tables 0 -> 2, 1 -> 3
    "seq_tables_2_3": (lambda: renumbered(_arith(["-revert"]), {0: 2, 1: 3}), False),
    # statistics extremes: large magnitudes and the magnitude bins above Kx; long end-of-block runs and 129 chains
    "seq_noise_q100": (lambda: _arith(["-revert", "-quality", "100"], TC.noise(64, 64, 11)), False),
    "prog_noise_q100": (lambda: _arith(SIMPLE + ["-quality", "100"], TC.noise(64, 64, 11)), True),
    "seq_flat_restart1": (lambda: _arith(["-revert", "-grayscale", "-restart", "1"], PC.flat_gray()), False),
    # four components
    "ycck_420": (ycck_arith, False),
}
NAMES = list(SOURCES)
FOUR = ["ycck_420"]
THREE = [n for n in NAMES if n not in FOUR]


@functools.lru_cache(maxsize=None)
def source(name):
    if name == "incomplete":
        return _arith(["-revert"], script=PC.SCRIPT_INCOMPLETE)
    return SOURCES[name][0]()


def kw_of(name):
    return dict(arithmetic_sources=True, progressive_sources=name == "incomplete" or SOURCES[name][1])


@functools.lru_cache(maxsize=None)
def ref_coefs(jpeg):
    rc, text, data = CC.dump_files(O.REF_DIR, "dump", [jpeg])
    assert rc == 0 and data, "coef_dump on the reference's library: %d\n%s" % (rc, text)
    return CC.parse_dump(data)


def _raise(x):
    if isinstance(x, Exception):
        raise x
    return x


# ---- 1. coefficients, pixels, planes, files -----------------------------------------------------------------------------------------------
def check_coefficients(M, name):
    src = source(name)
    out = _raise(M.decode_coefficients([src], **kw_of(name))[0])
    ref = ref_coefs(src)
    assert CC.same_arrays(out, ref), "%s, the reference %s" % ([a.shape for a in out], [a.shape for a in ref])
    if name == "seq_tables_2_3":      # the renumbered file is another file with the same coefficients
        assert src != source("seq_420") and CC.same_arrays(ref, ref_coefs(source("seq_420")))
    if name == "seq_flat_restart1":
        assert ref[0].shape[:2] == (129, 256) and not ref[0][..., 1:].any()


def check_pixels(M, name):
    src = source(name)
    out = _raise(M.decode([src], **kw_of(name))[0])
    if name in FOUR:
        rc, ref, text = CK.tj_pixels(src)
        assert rc == 0, text
        assert CK.same(out, ref)
    else:
        assert np.array_equal(out, DC.djpeg(src))


OPTION_SOURCES = ["seq_420", "prog_script_a", "seq_restart_rows"]


def check_pixel_options(M, name):
    src, kw = source(name), kw_of(name)
    assert np.array_equal(_raise(M.decode([src], scale=(1, 2), **kw)[0]), DC.djpeg(src, ["-scale", "1/2"]))
    assert np.array_equal(_raise(M.decode([src], dct="fast", **kw)[0]), DC.djpeg(src, ["-dct", "fast"]))
    assert DJ.same565(_raise(M.decode([src], color="rgb565", **kw)[0]), DJ.djpeg565(src))
    assert np.array_equal(_raise(M.decode([src], bottom_up=True, **kw)[0]), DC.djpeg(src)[::-1])


PLANE_SOURCES = ["seq_420", "prog_simple"]


def reference_planes(jpeg):
    """the planes of the reference's tj3DecompressToYUVPlanes8, tight strides (fast_idct_cases.reference_planes on these bytes)"""
    L = FI.tj()
    h = L.tj3Init(FI.TJINIT_DECOMPRESS)
    try:
        assert L.tj3DecompressHeader(h, jpeg, len(jpeg)) == 0
        sub, w, ht = (L.tj3Get(h, p) for p in (FI.TJPARAM_SUBSAMP, FI.TJPARAM_JPEGWIDTH, FI.TJPARAM_JPEGHEIGHT))
        assert sub >= 0
        planes = [np.full((L.tj3YUVPlaneHeight(c, ht, sub), L.tj3YUVPlaneWidth(c, w, sub)), 0xA5, np.uint8) for c in range(3)]
        ptrs = (C.c_void_p * 3)(*[p.ctypes.data for p in planes])
        assert L.tj3DecompressToYUVPlanes8(h, jpeg, len(jpeg), ptrs, None) == 0
        return planes
    finally:
        L.tj3Destroy(h)


def check_planes(M, name):
    src = source(name)
    out = _raise(M.decode_planes([src], **kw_of(name))[0])
    ref = reference_planes(src)
    assert len(out) == len(ref) == 3
    for a, b in zip(out, ref):
        assert FI.same(a, b), "%s against the reference's %s" % (a.shape, b.shape)


# jpegtran's switches: name -> (keywords of recompress, the program's arguments)
RECOMPRESS = {
    "revert_opt": (dict(revert=True, optimize=True), ["-revert", "-optimize"]),
    "progressive": (dict(progressive=True), ["-progressive"]),
    "default": (dict(), []),
    "revert_arith": (dict(revert=True, arithmetic=True), ["-revert", "-arithmetic"]),
}


def check_recompress(M, name, sw):
    src = source(name)
    kw, args = RECOMPRESS[sw]
    out = _raise(M.recompress([src], **kw, **kw_of(name))[0])
    assert out == O.ref_jpegtran(src, ["-copy", "none"] + args)


def with_markers(jpeg):
    """a COM and an Exif-less APP1 behind the file's APP0"""
    assert jpeg[2:4] == b"\xff\xe0"
    at = 4 + ((jpeg[4] << 8) | jpeg[5])
    com, app1 = b"arithmetic source", b"http://ns.adobe.com/xap/1.0/\0<x/>"
    seg = lambda m, d: bytes([0xFF, m, (len(d) + 2) >> 8, (len(d) + 2) & 255]) + d
    return jpeg[:at] + seg(0xFE, com) + seg(0xE1, app1) + jpeg[at:]


def check_marker_copy(M):
    src = with_markers(source("seq_420"))
    assert [m for m, _ in M.jpeg_markers(src, "all", arithmetic_sources=True)] == [0xE0, 0xFE, 0xE1]
    for sw in ("revert_opt", "revert_arith"):
        kw, args = RECOMPRESS[sw]
        out = _raise(M.recompress([src], copy="all", arithmetic_sources=True, **kw)[0])
        assert out == O.ref_jpegtran(src, ["-copy", "all"] + args), sw


def check_mixed_batch(M):
    """a Huffman sequential, a Huffman progressive, an SOF9 and an SOF10 file of one geometry in one call"""
    files = [TC.cjpeg(TC.testorig(), ["-revert"]), TC.cjpeg(PC.second_image(), ["-revert", "-progressive"]), source("seq_420"),
             _arith(SIMPLE, PC.second_image())]
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True, optimize=True), max_batch=4)
    enc.set_sources(progressive=True, arithmetic=True)
    try:
        co = enc.decode_host(files, coefficients=True)
        st = enc.arith_stats()
        nscans = len(M.jpeg_info(files[3], True, False, True).prog_scans)
        assert st["chains"] == 1 + nscans and st["launches"] == 1 + nscans, st
        huff = [(tuple(p.component_index[:p.comps_in_scan]), p.Ss, p.Se, p.Ah, p.Al) for p in M.jpeg_info(files[1], True).prog_scans]
        assert enc.prog_stats()["levels"] == PC.levels_of(huff) > 1      # (the Huffman-coded progressive file's: its meaning is kept)
        for i, f in enumerate(files):
            assert CC.same_arrays(co[i], ref_coefs(f)), i
        pix = enc.decode_host(files)
        for i, f in enumerate(files):
            assert np.array_equal(pix[i], DC.djpeg(f)), i
        rec = enc.transcode_host(files)
        for i, f in enumerate(files):
            assert rec[i] == O.ref_jpegtran(f, ["-copy", "none", "-revert", "-optimize"]), i
        enc.decode_host(files[:2], coefficients=True)     # a call without an arithmetic file reports none
        assert enc.arith_stats() == dict(chains=0, launches=0, ms=0.0)
    finally:
        enc.close()


# ---- 2. damaged data --------------------------------------------------------------------------------------------------------------------
# Found on the CPU with the reference's djpeg: these 32 bytes at offset 2041 of seq_420's entropy-coded data make it report
# "Corrupt JPEG data: bad arithmetic code" (JWRN_ARITH_BAD_CODE).  (Most overwrites leave a stream that decodes to the end without an
# overflow; the reference then warns about the bytes left over, if about anything.)
BAD_CODE_AT = 2041
BAD_CODE_BYTES = bytes.fromhex("c011ed201f836320adb98bab1686a28d9801210c7736f3eec580dcfc43fe5d04")


def djpeg_messages(jpeg):
    with tempfile.TemporaryDirectory() as td:
        inp = os.path.join(td, "in.jpg")
        with open(inp, "wb") as f:
            f.write(jpeg)
        r = subprocess.run([DC.DJPEG, "-outfile", os.path.join(td, "out.ppm"), inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        return r.returncode, r.stderr.decode(errors="replace")


def bad_code_file(M):
    src = source("seq_420")
    s = M.jpeg_info(src, arithmetic_sources=True).scans[0]
    assert BAD_CODE_AT + len(BAD_CODE_BYTES) < s.data_size
    a = s.data_offset + BAD_CODE_AT
    return src[:a] + BAD_CODE_BYTES + src[a + len(BAD_CODE_BYTES):]


def check_bad_code_in_a_batch(M):
    bad, good, other = bad_code_file(M), source("seq_420"), _arith(["-revert"], PC.second_image())
    rc, text = djpeg_messages(bad)
    assert rc == 2 and "bad arithmetic code" in text, (rc, text)
    files = [good, bad, other]
    for fn in (M.decode_coefficients, M.decode):
        out = fn(files, arithmetic_sources=True, max_batch=3)
        assert isinstance(out[1], M.MjhError) and out[1].code == M.EINVAL and "Corrupt JPEG data" in str(out[1]), out[1]
    out = M.decode_coefficients(files, arithmetic_sources=True, max_batch=3)
    assert CC.same_arrays(out[0], ref_coefs(good)) and CC.same_arrays(out[2], ref_coefs(other))
    rec = M.recompress(files, arithmetic_sources=True, max_batch=3, revert=True, optimize=True)
    assert isinstance(rec[1], M.MjhError) and rec[1].code == M.EINVAL, rec[1]
    for i in (0, 2):
        assert rec[i] == O.ref_jpegtran(files[i], ["-copy", "none", "-revert", "-optimize"]), i


def check_truncated(M):
    """the last bytes of the entropy-coded data cut, EOI kept: the reference is silent (zeros follow a marker), and so are we"""
    for name, cut in (("seq_420", 5), ("prog_simple", 3)):
        src, kw = source(name), kw_of(name)
        info = M.jpeg_info(src, kw["progressive_sources"], False, True)
        s = info.prog_scans[-1] if info.sof_type == 10 else info.scans[info.num_scans - 1]
        end = s.data_offset + s.data_size
        short = src[:end - cut] + src[end:]
        assert short[-2:] == b"\xff\xd9" and len(short) == len(src) - cut
        rc, text = djpeg_messages(short)
        assert rc == 0 and text.strip() == "", (name, rc, text)
        assert CC.same_arrays(_raise(M.decode_coefficients([short], **kw)[0]), ref_coefs(short)), name
        assert np.array_equal(_raise(M.decode([short], **kw)[0]), DC.djpeg(short)), name


# ---- 3. refusals and defaults -------------------------------------------------------------------------------------------------------------
def _refused(x, code, *words):
    assert isinstance(x, Exception), "accepted"
    assert x.code == code and all(w in str(x) for w in words), x


def _call(fn):
    try:
        fn()
    except Exception as exc:      # noqa: BLE001 (the refusal is what is looked at)
        return exc
    return None


def patched_sof(jpeg, marker):
    at = jpeg.index(b"\xff\xc9") if b"\xff\xc9" in jpeg[:400] else jpeg.index(b"\xff\xca")
    return jpeg[:at + 1] + bytes([marker]) + jpeg[at + 2:]


def patched_dac(jpeg, index=None, value=None):
    """the first (index, value) pair of the first DAC segment changed"""
    at = jpeg.index(b"\xff\xcc")
    b = bytearray(jpeg)
    if index is not None:
        b[at + 4] = index
    if value is not None:
        b[at + 5] = value
    return bytes(b)


def check_refusals(M):
    seq, prog = source("seq_420"), source("prog_simple")
    # without the flag: the words of before the feature, whatever else is set
    for kw in (dict(), dict(progressive_sources=True)):
        for src, n in ((seq, 9), (prog, 10)):
            _refused(_call(lambda: M.jpeg_info(src, **kw)), M.EUNSUPPORTED, "arithmetic-coded source file (SOF%d)" % n)
            for fn in (M.decode, M.decode_coefficients, M.decode_planes, M.recompress):
                x = fn([src], **kw)[0]
                _refused(x, M.EUNSUPPORTED, "arithmetic-coded source file (SOF%d)" % n)
                assert str(x).rstrip().endswith("arithmetic-coded source file (SOF%d)" % n), x
    # a DAC in front of the frame header (a Huffman-coded file that carries one) is answered with the DAC text
    huff = TC.cjpeg(TC.testorig(), ["-revert"])
    sof = huff.index(b"\xff\xc0")
    with_dac = huff[:sof] + b"\xff\xcc\x00\x04\x00\x10" + huff[sof:]
    x = _call(lambda: M.jpeg_info(with_dac))
    _refused(x, M.EUNSUPPORTED, "arithmetic-coding conditioning (DAC) in the source file")
    assert str(x).rstrip().endswith("arithmetic-coding conditioning (DAC) in the source file")
    # ... and with the flag it is read and ignored, as the reference does
    assert np.array_equal(DC.djpeg(with_dac), DC.djpeg(huff))
    assert CC.same_arrays(_raise(M.decode_coefficients([with_dac], arithmetic_sources=True)[0]), ref_coefs(huff))
    # SOF10 without progressive_sources names the missing flag
    _refused(_call(lambda: M.jpeg_info(prog, arithmetic_sources=True)), M.EUNSUPPORTED, "SOF10", "MJH_SRC_PROGRESSIVE")
    _refused(M.decode_coefficients([prog], arithmetic_sources=True)[0], M.EUNSUPPORTED, "SOF10", "MJH_SRC_PROGRESSIVE")
    # SOF11, table 4, L > U, an index outside 0..31
    both = dict(arithmetic_sources=True, progressive_sources=True)
    _refused(_call(lambda: M.jpeg_info(patched_sof(seq, 0xCB), **both)), M.EUNSUPPORTED, "SOF11")
    t4 = renumbered(seq, {1: 4})
    _refused(_call(lambda: M.jpeg_info(t4, **both)), M.EUNSUPPORTED, "conditioning table 4")
    _refused(M.decode_coefficients([t4], **both)[0], M.EUNSUPPORTED, "conditioning table 4")
    rc, _ = djpeg_messages(t4)
    assert rc == 0                                       # (the reference takes tables 0..15)
    _refused(_call(lambda: M.jpeg_info(patched_dac(seq, value=0x12), **both)), M.EINVAL, "JERR_DAC_VALUE")
    _refused(_call(lambda: M.jpeg_info(patched_dac(seq, index=0x20), **both)), M.EINVAL, "JERR_DAC_INDEX")
    # a transform
    enc = M.Encoder(M.params_from_jpeg(huff, revert=True, transform="flip_h"), max_batch=1)
    enc.set_sources(progressive=True, arithmetic=True)
    try:
        assert enc.transcode_host([huff])[0] == O.ref_jpegtran(huff, ["-copy", "none", "-revert", "-flip", "horizontal"])
        for src in (seq, prog):
            _refused(_call(lambda: enc.transcode_host([src])), M.EUNSUPPORTED, "transform", "arithmetic")
    finally:
        enc.close()
    # an encoder made from a lossless file's parameters decodes lossless files alone and does not know the bit (SOF11 is not decoded);
    # decode() with both keywords still reads a lossless file
    ll = TC.cjpeg(TC.testorig(), ["-revert", "-lossless", "1"])
    assert np.array_equal(_raise(M.decode([ll], lossless_sources=True, arithmetic_sources=True)[0]), DC.djpeg(ll))
    enc = M.Encoder(M.params_from_jpeg(ll, revert=True, lossless_sources=True), max_batch=1)
    try:
        _refused(_call(lambda: enc.set_sources(progressive=False, lossless=True, arithmetic=True)), M.EINVAL, "lossless encoder", "SOF11")
        enc.set_sources(progressive=False, lossless=True)
    finally:
        enc.close()
    enc = M.Encoder(M.params_from_jpeg(huff, revert=True), max_batch=1)
    try:
        _refused(_call(lambda: enc.decode_host([seq], coefficients=True)), M.EUNSUPPORTED, "arithmetic-coded source file (SOF9)")
        enc.set_sources(progressive=False, arithmetic=True)
        assert CC.same_arrays(enc.decode_host([seq], coefficients=True)[0], ref_coefs(seq))
        enc.set_sources(progressive=False)
        _refused(_call(lambda: enc.decode_host([seq], coefficients=True)), M.EUNSUPPORTED, "arithmetic-coded source file (SOF9)")
    finally:
        enc.close()


def check_incomplete_script(M):
    """an SOF10 file whose blocks djpeg would smooth: coefficients and files as the reference's, no pixels and no planes"""
    src, kw = source("incomplete"), kw_of("incomplete")
    assert CC.same_arrays(_raise(M.decode_coefficients([src], **kw)[0]), ref_coefs(src))
    assert _raise(M.recompress([src], revert=True, optimize=True, **kw)[0]) == O.ref_jpegtran(src, ["-copy", "none", "-revert", "-optimize"])
    for out in (M.decode([src], **kw)[0], M.decode_planes([src], **kw)[0]):
        _refused(out, M.EUNSUPPORTED, "block smoothing")


# ---- 4. probing -------------------------------------------------------------------------------------------------------------------------
def check_probe(M):
    seq = M.jpeg_info(source("seq_420"), arithmetic_sources=True)
    assert seq.sof_type == 9 and seq.num_scans == 1 and seq.prog_scans == []
    s = seq.scans[0]
    assert s.huff_defined == 0 and list(s.dc_tbl_no[:3]) == [0, 1, 1] and list(s.ac_tbl_no[:3]) == [0, 1, 1]
    assert seq.arith_cond == [dict(dc_L=[0] * 4, dc_U=[1] * 4, ac_K=[5] * 4)]
    cond = M.jpeg_info(source("seq_cond"), arithmetic_sources=True)
    assert cond.arith_cond == [dict(dc_L=[1, 0, 0, 0], dc_U=[3, 2, 1, 1], ac_K=[9, 20, 5, 5])]
    moved = M.jpeg_info(source("seq_tables_2_3"), arithmetic_sources=True)
    assert list(moved.scans[0].dc_tbl_no[:3]) == [2, 3, 3] and list(moved.scans[0].ac_tbl_no[:3]) == [2, 3, 3]
    prog = M.jpeg_info(source("prog_cond"), progressive_sources=True, arithmetic_sources=True)
    assert prog.sof_type == 10 and prog.num_scans == 0 and len(prog.prog_scans) == len(prog.arith_cond) > 1
    assert all(p.huff_defined == 0 for p in prog.prog_scans)
    # a table keeps its conditioning from scan to scan: the last scan still sees what the DAC in front of an earlier one set
    assert prog.arith_cond[-1]["dc_L"][:2] == [0, 3] and prog.arith_cond[-1]["dc_U"][:2] == [15, 4]
    assert any(c["ac_K"][:2] == [12, 2] for c in prog.arith_cond)
    got = [(tuple(p.component_index[:p.comps_in_scan]), p.Ss, p.Se, p.Ah, p.Al) for p in
           M.jpeg_info(source("prog_script_a"), progressive_sources=True, arithmetic_sources=True).prog_scans]
    assert got == PC.parse_script(PC.SCRIPT_A)
    # a Huffman-coded file: the same answer with and without the flag
    huff = TC.cjpeg(TC.testorig(), ["-revert"])
    assert bytes(M.jpeg_info(huff)) == bytes(M.jpeg_info(huff, arithmetic_sources=True))
    # the caller's room counts
    f = source("seq_420")
    n = C.c_int()
    assert M.lib().mjh_jpeg_arith_cond(f, len(f), M.SRC_ARITHMETIC, None, 0, C.byref(n)) == M.EINVAL and n.value == 1
    assert M.lib().mjh_jpeg_arith_cond(f, len(f), 0, None, 0, C.byref(n)) == M.EUNSUPPORTED
