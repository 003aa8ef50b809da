"""Host model of the MSM's signed lazy-limb arithmetic under AddressSanitizer + UndefinedBehaviorSanitizer: csrc/lazy29.hpp and
csrc/msm_kernels.hpp compiled as plain C++ and run against the CPU oracle on the inputs their range and no-overflow arguments are tightest
on (tests/sanitize/lazy_bucket_main.cpp lists the checks).  An overflowing int64 column sum or int32 limb sum, silent on the GPU, is a UBSan
report here and aborts the program.  No GPU involved, nothing of the product library linked."""
import os
import subprocess

import msm_edges
from oracle_lib import ROOT

SAN = os.path.join(ROOT, "tests", "sanitize")


def test_lazy_bucket_arithmetic_under_asan_ubsan(tmp_path):
    subprocess.check_call(["make", "-j3", "-C", SAN, "-f", "lazy_bucket.mk"], stdout=subprocess.DEVNULL, timeout=1200)
    edges = str(tmp_path / "edge_points.bin")
    counts = msm_edges.write_edge_file(edges)          # first points of check 4's chains: curve points on unpack_small's boundary values
    assert min(counts) > 1000
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([os.path.join(SAN, "_build", "lazy_bucket_main"), edges], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-6000:]
    assert "\n0 failure(s)" in p.stdout
    assert "edge first points: " + " + ".join(str(c) for c in counts) + "\n" in p.stdout      # the program read all four tables
    for k in range(1, 6):
        assert f"check {k}:" in p.stdout
