"""CPU suite: the arithmetic decoder core (mozjpeg_amd/csrc/mjh_arith_decoder.h) compiled for the host -- a "vector register" is an
array of 64 ints -- and run by tests/native/arith_decoder_check.cpp: the product's host-compiled coder writes random scans of the
five kinds (restarts, random conditioning, table numbers 0..3), the decoder reads them back, and coefficients, final statistics bins,
registers and bytes consumed must agree with what was coded and with a plain restatement of the reference's decoder; segments cut
short are continued with zeros; hand-made streams drive every overflow branch to the bad-code state."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_compiled_decoder_reads_back_what_the_coder_wrote(tmp_path):
    exe = str(tmp_path / "arith_decoder_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "arith_decoder_check.cpp")])
    for args in (["400", "12345"], ["150", "7"]):
        r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        text = r.stdout.decode(errors="replace")
        assert r.returncode == 0, text[-3000:]
        assert "7 of 7 overflow branches reached: identical" in text, text[-3000:]
