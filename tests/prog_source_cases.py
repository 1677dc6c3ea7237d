"""The case list and helpers of the progressive-source tests (test_simt_prog_sources.py on the emulator, test_gpu_prog_sources.py on
the chip): Huffman-coded progressive files (SOF2) through mozjpeg_amd.decode_coefficients, decode and recompress with
progressive_sources=True, i.e. mjh_jpeg_probe_ex, mjh_encoder_set_sources and the kernels of mjh_decode_prog.hip.

Every source is written by the reference's cjpeg at test time (transcode_cases.cjpeg, with script= for -scans); every expected value
comes from the reference at test time: coefficient arrays from tests/native/coef_dump on oracle/_ref/libjpeg.so.62, pixels from
djpeg, files from jpegtran -copy none.  Every comparison is exact equality.

Two things about the sources that are not obvious:
  * `cjpeg -restart 1` in the default (max-compression) profile writes its DRI once, in front of the first scan, although the
    interval in MCUs differs between the interleaved DC scan and the luma AC scans; the reference's own djpeg and jpegtran exit with
    warnings on that file.  The restart-in-rows case therefore uses -revert -progressive, where a DRI precedes every scan whose
    interval changes and the reference reads its own file cleanly.  -restart 3B is used with both profiles.
  * the default profile's scan search keeps successive approximation only where it pays; for testorig it does not, so the cases
    that are about refinement scans (damaged input, subsequence lengths) use -revert -progressive (jpeg_simple_progression)."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":          # a child process of check_subsequence_lengths: the package lies next to tests/
    sys.path.insert(0, ROOT)

import oracle_lib as O
import coef_cases as CC
import decode_cases as DC
import transcode_cases as TC


def have_tools():
    return CC.have_tools() and DC.have_tools()


# DC in three steps (Al 2, 1, 0) with one DC scan per component, AC in the bands 1-5 / 6-63, three AC approximation steps (2 -> 1 -> 0),
# the last luma step over the merged band: levels 0, 1, 2
SCRIPT_A = """0: 0 0 0 2;
1: 0 0 0 2;
2: 0 0 0 2;
0: 1 5 0 2;
0: 6 63 0 2;
1: 1 63 0 2;
2: 1 63 0 2;
0: 0 0 2 1;
1: 0 0 2 1;
2: 0 0 2 1;
0: 1 5 2 1;
0: 6 63 2 1;
1: 1 63 2 1;
2: 1 63 2 1;
0,1,2: 0 0 1 0;
0: 1 63 1 0;
1: 1 63 1 0;
2: 1 63 1 0;
"""
# another level structure: one interleaved DC scan in two steps, luma AC in two steps, chroma AC at once: levels 0, 1
SCRIPT_B = """0,1,2: 0 0 0 1;
0: 1 63 0 1;
1: 1 63 0 0;
2: 1 63 0 0;
0,1,2: 0 0 1 0;
0: 1 63 1 0;
"""
# DC of every component, luma AC at Al = 1 with no refinement, no chroma AC: the reference's djpeg smooths its blocks
SCRIPT_INCOMPLETE = """0,1,2: 0 0 0 0;
0: 1 63 0 1;
"""
# the most scans cjpeg writes (rdswitch.c MAX_SCANS = 64): DC + 63 luma scans of one coefficient each; and the chroma AC scans that
# sixty_six_scans() splices behind them
SCRIPT_64 = "0,1,2: 0 0 0 0;\n" + "".join("0: %d %d 0 0;\n" % (k, k) for k in range(1, 64))
SCRIPT_CHROMA = "0,1,2: 0 0 0 0;\n1: 1 63 0 0;\n2: 1 63 0 0;\n"


def parse_script(text):
    """[(components, Ss, Se, Ah, Al), ...] of a -scans file"""
    out = []
    for entry in text.replace("\n", " ").split(";"):
        if entry.strip():
            comps, rest = entry.split(":")
            out.append((tuple(int(c) for c in comps.split(",")),) + tuple(int(v) for v in rest.split()))
    return out


def levels_of(scans):
    """how many levels of scans a script has: first scans are level 0; a refinement is one above the highest earlier scan that shares a
    component and overlaps its coefficient range"""
    lv = []
    for k, (comps, ss, se, ah, al) in enumerate(scans):
        v = 0
        if ah:
            for t in range(k):
                c2, s2, e2 = scans[t][:3]
                if set(comps) & set(c2) and s2 <= se and ss <= e2:
                    v = max(v, lv[t] + 1)
        lv.append(v)
    return max(lv) + 1


def flat_gray():
    return np.full((1032, 2048, 3), 128, np.uint8)


def second_image():
    return np.ascontiguousarray(TC.testorig()[::-1, ::-1])


# name -> maker.  The smallest sources at which each mechanism can go wrong: the two profiles' own scripts on 227 x 149 in 4:2:0, 4:4:4,
# 2x1 and gray; partial MCUs where the non-interleaved raster is narrower than the interleaved grid (17 x 9 at 2x1), a single MCU and a
# single pixel; restart intervals that differ from scan to scan; the two hand-written scripts; EOB runs that hit the coder's 0x7FFF
# cap (33 024 flat blocks); long code words, correction bits on almost every position and ZRL inside refinement (noise at quality 100)
SOURCES = {
    "default_420": lambda: TC.cjpeg(TC.testorig(), ["-quality", "75"]),
    "simple_420": lambda: TC.cjpeg(TC.testorig(), ["-revert", "-progressive"]),
    "default_444": lambda: TC.cjpeg(TC.testorig(), ["-sample", "1x1"]),
    "simple_444": lambda: TC.cjpeg(TC.testorig(), ["-revert", "-progressive", "-sample", "1x1"]),
    "default_2x1": lambda: TC.cjpeg(TC.testorig(), ["-sample", "2x1"]),
    "simple_2x1": lambda: TC.cjpeg(TC.testorig(), ["-revert", "-progressive", "-sample", "2x1"]),
    "default_gray": lambda: TC.cjpeg(TC.testorig(), ["-grayscale"]),
    "simple_gray": lambda: TC.cjpeg(TC.testorig(), ["-revert", "-progressive", "-grayscale"]),
    "17x9_2x1_default": lambda: TC.cjpeg(O.synthetic_frame(17, 9, 5), ["-sample", "2x1"]),
    "17x9_2x1_simple": lambda: TC.cjpeg(O.synthetic_frame(17, 9, 5), ["-revert", "-progressive", "-sample", "2x1"]),
    "8x8_default": lambda: TC.cjpeg(O.synthetic_frame(8, 8, 4), []),
    "8x8_simple": lambda: TC.cjpeg(O.synthetic_frame(8, 8, 4), ["-revert", "-progressive"]),
    "1x1_default": lambda: TC.cjpeg(O.synthetic_frame(1, 1, 3), []),
    "1x1_simple": lambda: TC.cjpeg(O.synthetic_frame(1, 1, 3), ["-revert", "-progressive"]),
    "restart_rows": lambda: TC.cjpeg(TC.testorig(), ["-revert", "-progressive", "-restart", "1"]),
    "restart_3b_default": lambda: TC.cjpeg(TC.testorig(), ["-restart", "3B"]),
    "restart_3b_simple": lambda: TC.cjpeg(TC.testorig(), ["-revert", "-progressive", "-restart", "3B"]),
    "script_a": lambda: TC.cjpeg(TC.testorig(), ["-revert"], script=SCRIPT_A),
    "script_b": lambda: TC.cjpeg(TC.testorig(), ["-revert"], script=SCRIPT_B),
    "script_a_restart_2": lambda: TC.cjpeg(TC.testorig(), ["-revert", "-restart", "2"], script=SCRIPT_A),
    "flat": lambda: TC.cjpeg(flat_gray(), ["-revert", "-progressive", "-grayscale"]),
    "noise_q100": lambda: TC.cjpeg(TC.noise(64, 64, 11), ["-revert", "-progressive", "-quality", "100"]),
}
# cases that would take the emulator minutes run on the chip only: none -- the flat image's 33 024 blocks take it about a second
GPU_ONLY = []
NAMES = list(SOURCES)


@functools.lru_cache(maxsize=None)
def source(name):
    if name == "incomplete":
        return TC.cjpeg(TC.testorig(), ["-revert"], script=SCRIPT_INCOMPLETE)
    return SOURCES[name]()


@functools.lru_cache(maxsize=None)
def ref_coefs(jpeg):
    rc, text, data = CC.dump_files(O.REF_DIR, "dump", [jpeg])
    assert rc == 0 and data, "coef_dump on the reference's library: %d\n%s" % (rc, text)
    return CC.parse_dump(data)


# ---- 1. the three paths -----------------------------------------------------------------------------------------------------------------
def check_coefficients(M, name):
    src = source(name)
    out = M.decode_coefficients([src], progressive_sources=True)[0]
    if isinstance(out, Exception):
        raise out
    ref = ref_coefs(src)
    assert CC.same_arrays(out, ref), "%s, the reference %s" % ([a.shape for a in out], [a.shape for a in ref])
    if name == "flat":
        assert ref[0].shape[:2] == (129, 256) and not ref[0][..., 1:].any()        # the case is what it says: 33 024 blocks, every AC scan EOB runs


PIXEL_MODES = {
    "default": (dict(), []),
    "nosmooth": (dict(fancy_upsampling=False), ["-nosmooth"]),
    "grayscale": (dict(color="gray"), ["-grayscale"]),
    "scale_1_2": (dict(scale="1/2"), ["-scale", "1/2"]),
    "dct_fast": (dict(dct="fast"), ["-dct", "fast"]),
}


def check_pixels(M, name, mode="default"):
    src = source(name)
    kw, args = PIXEL_MODES[mode]
    out = M.decode([src], progressive_sources=True, **kw)[0]
    if isinstance(out, Exception):
        raise out
    assert np.array_equal(out, DC.djpeg(src, args))


RECOMPRESS_SWITCHES = ["default", "revert_opt", "progressive"]       # of transcode_cases.SWITCHES


def check_recompress(M, name, sw):
    src = source(name)
    kw, args = TC.SWITCHES[sw]
    out = M.recompress([src], progressive_sources=True, **kw)[0]
    if isinstance(out, Exception):
        raise out
    assert out == O.ref_jpegtran(src, ["-copy", "none"] + args)


def check_incomplete_script(M):
    """coefficients and re-compression as the reference's; on the way to pixels and planes the refusal that names block smoothing"""
    check_coefficients(M, "incomplete")
    check_recompress(M, "incomplete", "default")
    check_recompress(M, "incomplete", "revert_opt")
    src = source("incomplete")
    for out in (M.decode([src], progressive_sources=True)[0], M.decode_planes([src], progressive_sources=True)[0]):
        assert isinstance(out, M.MjhError) and out.code == M.EUNSUPPORTED and "block smoothing" in str(out), out


# ---- 2. one call, eight files -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch_files():
    """two scripts x progressive and sequential x two images of one geometry, all with the tables of -revert"""
    out = []
    for img in (TC.testorig(), second_image()):
        out += [TC.cjpeg(img, ["-revert"], script=SCRIPT_A), TC.cjpeg(img, ["-revert"]), TC.cjpeg(img, ["-revert"], script=SCRIPT_B),
                TC.cjpeg(img, ["-revert"], script=TC.SCRIPT_3)]
    return out


def check_batch_of_eight(M):
    files = batch_files()
    enc = M.Encoder(M.params_from_jpeg(files[0], revert=True, optimize=True, progressive_sources=True), max_batch=8)
    enc.set_sources(progressive=True)
    try:
        co = enc.decode_host(files, coefficients=True)
        assert enc.prog_stats()["levels"] == max(levels_of(parse_script(SCRIPT_A)), levels_of(parse_script(SCRIPT_B))) == 3
        for i, f in enumerate(files):
            assert CC.same_arrays(co[i], ref_coefs(f)), i
        pix = enc.decode_host(files)
        for i, f in enumerate(files):
            assert np.array_equal(pix[i], DC.djpeg(f)), i
        rec = enc.transcode_host(files)
        for i, f in enumerate(files):
            assert rec[i] == O.ref_jpegtran(f, ["-copy", "none", "-revert", "-optimize"]), i
        # a call without a progressive file reports no level; the two scripts alone report their own
        enc.decode_host([files[1], files[3]], coefficients=True)
        assert enc.prog_stats()["levels"] == 0
        enc.decode_host([files[2]], coefficients=True)
        assert enc.prog_stats()["levels"] == levels_of(parse_script(SCRIPT_B)) == 2
        enc.decode_host([files[0]], coefficients=True)
        assert enc.prog_stats()["levels"] == 3
    finally:
        enc.close()


# ---- 3. the subsequence length (read at encoder creation: a child process per value) --------------------------------------------------------
def _digest(arrays, recoded, pixels):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(recoded)
    h.update(np.ascontiguousarray(pixels).tobytes())
    return h.hexdigest()


def child_main(lib_path, strict):
    """what a child process of check_subsequence_lengths prints: a digest of the three results and the synchronisation rounds"""
    import mozjpeg_amd as M
    if lib_path:
        M.LIB_PATH, M._lib = lib_path, None
    if strict:
        os.environ["SIMT_STRICT"] = "1"
    src = source("simple_420")
    enc = M.Encoder(M.params_from_jpeg(src, revert=True, progressive_sources=True), max_batch=1)
    enc.set_sources(progressive=True)
    co = enc.decode_host([src], coefficients=True)[0]
    st = enc.transcode_stats()
    pix = enc.decode_host([src])[0]
    rec = enc.transcode_host([src])[0]
    print(json.dumps(dict(digest=_digest(co, rec, pix), rounds=st["rounds"], subseq=st["subseq"])))


def check_subsequence_lengths(M):
    """the children load the library this process uses (the emulator's, with its strict mode, when the tests run on it)"""
    lib_path, strict = M.LIB_PATH, bool(os.environ.get("SIMT_STRICT"))
    src = source("simple_420")
    want = _digest(ref_coefs(src), O.ref_jpegtran(src, ["-copy", "none", "-revert"]), DC.djpeg(src))
    for subseq in (16, 0):
        env = dict(os.environ, MJH_DECODE_SUBSEQ=str(subseq))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib_path or "", "1" if strict else ""], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=os.path.join(ROOT, "tests"))
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
        got = json.loads(r.stdout.decode().strip().split("\n")[-1])
        assert got["subseq"] == subseq
        assert got["digest"] == want, "MJH_DECODE_SUBSEQ=%d" % subseq
        if subseq == 16:
            assert got["rounds"] > 0, got


# ---- 4. the marker walk -----------------------------------------------------------------------------------------------------------------
def check_prog_scans(M):
    for name, script in (("script_a", SCRIPT_A), ("script_b", SCRIPT_B), ("incomplete", SCRIPT_INCOMPLETE)):
        info = M.jpeg_info(source(name), progressive_sources=True)
        assert info.sof_type == 2 and info.num_scans == 0
        got = [(tuple(s.component_index[:s.comps_in_scan]), s.Ss, s.Se, s.Ah, s.Al) for s in info.prog_scans]
        assert got == parse_script(script), name
    # a sequential file: the same answer with and without the keyword, no extended scans
    seq = TC.source("revert")
    a, b = M.jpeg_info(seq), M.jpeg_info(seq, progressive_sources=True)
    assert bytes(a) == bytes(b) and b.prog_scans == [] and b.sof_type == 0 and b.num_scans == 1


@functools.lru_cache(maxsize=None)
def sixty_six_scans():
    """more scans than MJH_MAX_SRC_SCANS (64), which is also the most cjpeg writes: the 64 scans of SCRIPT_64, and behind them the two
    chroma AC scans (with their DHT segments) of the same image coded with SCRIPT_CHROMA"""
    import mozjpeg_amd as M
    a = TC.cjpeg(TC.testorig(), ["-revert"], script=SCRIPT_64)
    b = TC.cjpeg(TC.testorig(), ["-revert"], script=SCRIPT_CHROMA)
    dc = M.jpeg_info(b, progressive_sources=True).prog_scans[0]
    assert a[-2:] == b[-2:] == b"\xff\xd9"
    return a[:-2] + b[dc.data_offset + dc.data_size:]


def check_too_many_scans(M):
    src = sixty_six_scans()
    full = TC.cjpeg(TC.testorig(), ["-revert"], script=SCRIPT_CHROMA + "0: 1 63 0 0;\n")
    assert np.array_equal(DC.djpeg(src), DC.djpeg(full))                  # the reference reads it, and as the same image
    for call in (lambda: M.jpeg_info(src, progressive_sources=True), lambda: _raise(M.decode_coefficients([src], progressive_sources=True)[0])):
        try:
            call()
            raise AssertionError("66 scans were accepted")
        except M.MjhError as exc:
            assert exc.code == M.EUNSUPPORTED and "66 scans" in str(exc), exc
    # 64 scans are read
    check = TC.cjpeg(TC.testorig(), ["-revert"], script=SCRIPT_64)
    assert len(M.jpeg_info(check, progressive_sources=True).prog_scans) == 64
    assert CC.same_arrays(_raise(M.decode_coefficients([check], progressive_sources=True)[0]), ref_coefs(check))
    # the caller's own room counts as well
    import ctypes as C
    info, room, n = M.JpegInfo(), (M.JpegScanEx * 8)(), C.c_int()
    f = source("script_a")
    assert M.lib().mjh_jpeg_probe_ex(f, len(f), M.SRC_PROGRESSIVE, C.byref(info), room, 8, C.byref(n)) == M.EUNSUPPORTED
    assert b"18 scans" in M.lib().mjh_last_error()


def _raise(x):
    if isinstance(x, Exception):
        raise x
    return x


def patch_sos(jpeg, scan, ss=None, se=None, ah=None, al=None):
    """the file with the last three bytes of scan `scan`'s SOS header (Ss, Se, Ah << 4 | Al) changed"""
    import mozjpeg_amd as M
    s = M.jpeg_info(jpeg, progressive_sources=True).prog_scans[scan]
    at = s.data_offset - 3
    b = bytearray(jpeg)
    assert (b[at], b[at + 1], b[at + 2]) == (s.Ss, s.Se, s.Ah << 4 | s.Al)
    b[at] = s.Ss if ss is None else ss
    b[at + 1] = s.Se if se is None else se
    b[at + 2] = (s.Ah if ah is None else ah) << 4 | (s.Al if al is None else al)
    return bytes(b)


def check_bogus_progressions(M):
    src = source("script_a")
    bad = {
        # scan 1 is component 1's DC scan: as an AC scan it comes before that component's DC
        "ac_before_dc": patch_sos(src, 1, ss=1, se=5),
        # scan 10 refines luma 1-5 from Al 2 to 1: as Ah 3 / Al 2 its Ah is not the Al before it (and Al = Ah - 1 still holds)
        "ah_not_previous_al": patch_sos(src, 10, ah=3, al=2),
        # scan 4 is the first scan of luma 6-63: as 1-63 it is a first scan of the coefficients 1-5 that scan 3 coded already
        "coded_twice": patch_sos(src, 4, ss=1, se=63),
    }
    for name, f in bad.items():
        for call in (lambda: M.jpeg_info(f, progressive_sources=True), lambda: _raise(M.decode_coefficients([f], progressive_sources=True)[0]),
                     lambda: _raise(M.recompress([f], progressive_sources=True)[0])):
            try:
                call()
                raise AssertionError("%s was accepted" % name)
            except M.MjhError as exc:
                assert exc.code == M.EUNSUPPORTED and "BOGUS_PROGRESSION" in str(exc), (name, exc)
    # what start_pass_phuff_decoder refuses outright: Al != Ah - 1 on a refinement
    try:
        M.jpeg_info(patch_sos(src, 10, ah=2, al=0), progressive_sources=True)
        raise AssertionError("Al != Ah - 1 was accepted")
    except M.MjhError as exc:
        assert exc.code == M.EINVAL and "JERR_BAD_PROGRESSION" in str(exc) and "Ss=1 Se=5 Ah=2 Al=0" in str(exc), exc


def check_default_refusals(M):
    """with nothing set, a progressive file is answered as before the feature: EUNSUPPORTED with the word progressive"""
    src = source("simple_420")

    def refused(x):
        assert isinstance(x, M.MjhError) and x.code == M.EUNSUPPORTED and "progressive" in str(x), x

    try:
        M.jpeg_info(src)
        raise AssertionError("jpeg_info took a progressive file")
    except M.MjhError as exc:
        refused(exc)
    refused(M.decode([src])[0])
    refused(M.decode_coefficients([src])[0])
    refused(M.decode_planes([src])[0])
    refused(M.recompress([src])[0])
    seq = TC.cjpeg(TC.testorig(), ["-revert"])
    enc = M.Encoder(M.params_from_jpeg(seq, revert=True), max_batch=2)
    try:
        def all_three():
            for call in (lambda: enc.transcode_host([src, seq]), lambda: enc.decode_host([src, seq]), lambda: enc.decode_host([src, seq], coefficients=True)):
                try:
                    call()
                    raise AssertionError("an encoder without set_sources took a progressive file")
                except M.MjhError as exc:
                    refused(exc)
        all_three()                                   # never given set_sources
        enc.set_sources(progressive=True)
        assert CC.same_arrays(enc.decode_host([src, seq], coefficients=True)[0], ref_coefs(src))
        enc.set_sources(progressive=False)
        all_three()                                   # and again after it was taken back
    finally:
        enc.close()


def check_transform_refused(M):
    src, seq = source("simple_420"), TC.cjpeg(TC.testorig(), ["-revert"])
    enc = M.Encoder(M.params_from_jpeg(seq, revert=True, transform="flip_h"), max_batch=1)
    enc.set_sources(progressive=True)
    try:
        assert enc.transcode_host([seq])[0] == O.ref_jpegtran(seq, ["-copy", "none", "-revert", "-flip", "horizontal"])
        try:
            enc.transcode_host([src])
            raise AssertionError("a transform together with a progressive file was accepted")
        except M.MjhError as exc:
            assert exc.code == M.EUNSUPPORTED and "progressive" in str(exc) and "transform" in str(exc), exc
    finally:
        enc.close()


# ---- 5. untrusted input -----------------------------------------------------------------------------------------------------------------
def scan_of(M, jpeg, ss, ah):
    """(offset, size) of the entropy-coded data of the first scan with this Ss (0 = DC) and this kind (ah: refinement or not)"""
    for s in M.jpeg_info(jpeg, progressive_sources=True).prog_scans:
        if (s.Ss == 0) == (ss == 0) and (s.Ah != 0) == ah:
            return s.data_offset, s.data_size
    raise AssertionError("no such scan")


def damaged_files(M):
    """simple_420 with 40 bytes cut out of, and the file ended inside, an AC first scan, a DC refinement and an AC refinement; and with
    20 seeded single-bit flips in its entropy-coded bytes"""
    import random
    src = source("simple_420")
    out = {}
    for kind, (ss, ah) in (("first", (1, False)), ("dc_refine", (0, True)), ("ac_refine", (1, True))):
        a, n = scan_of(M, src, ss, ah)
        out["cut_" + kind] = src[:a + n // 2] + src[a + n // 2 + min(40, n // 4):]
        out["end_" + kind] = src[:a + n // 2] + b"\xff\xd9"
    ranges = [(s.data_offset, s.data_size) for s in M.jpeg_info(src, progressive_sources=True).prog_scans]
    rng = random.Random(20240611)
    for i in range(20):
        a, n = ranges[rng.randrange(len(ranges))]
        bad = bytearray(src)
        bad[a + rng.randrange(n)] ^= 1 << rng.randrange(8)
        out["flip_%d" % i] = bytes(bad)
    return out


def check_damaged(M, names=None):
    """every call returns with a per-file status -- MJH_EINVAL for a damaged stream, or a decode -- and the good file of the same batch
    gives the reference's arrays"""
    src = source("simple_420")
    ref = ref_coefs(src)
    files = damaged_files(M)
    failed = 0
    for name in names or files:
        out = M.decode_coefficients([files[name], src], progressive_sources=True, max_batch=2)
        assert len(out) == 2
        if isinstance(out[0], Exception):
            assert isinstance(out[0], M.MjhError) and out[0].code == M.EINVAL, (name, out[0])
            failed += 1
        else:
            assert [a.shape for a in out[0]] == [a.shape for a in ref], name
        if name.startswith("end_") or name == "cut_dc_refine":         # fewer bits than blocks cannot decode
            assert isinstance(out[0], M.MjhError), name
        assert CC.same_arrays(out[1], ref), name
    return failed


if __name__ == "__main__" and len(sys.argv) >= 2 and sys.argv[1] == "--child":
    child_main(sys.argv[2] if len(sys.argv) > 2 else "", bool(sys.argv[3]) if len(sys.argv) > 3 else False)
