"""BFV Mul's host side (the one tensorAndRescale pipeline of lr_abi_bfv.cpp behind lr_bfv_mul and lr_bfv_mul_deg) under AddressSanitizer +
UBSan (CPU build only).  The product's host code -- every lattigo-fhe-by-go_amd/csrc/lr_*.cpp but lr_asm.cpp -- is
compiled with g++ against the host-only HIP stand-in and the recording launch stubs of tests/cpp/hipstub/ (host_stub_build.py), and driven by
tests/cpp/bfv_mul_deg_driver.cpp: every degree pair through lr_bfv_mul_deg, 1 x 1 through lr_bfv_mul as well, the squaring cases, batches on
both sides of the gather threshold, the paths without gathering and without the extension epilogues, aliased outputs and every refusal.  The
stubs touch the first and the last word of every row a kernel would read or write, so a wrong pool size, slot offset or stride is a
sanitizer report."""
from host_stub_build import ASAN_UBSAN, run_host_driver


def test_bfv_mul_deg_host_side_under_asan_ubsan(tmp_path):
    stdout, calls, refusals = run_host_driver(tmp_path, "bfv_mul_deg_driver", *ASAN_UBSAN)
    # 3 plans x 3 batches x (lr_bfv_mul_deg: 20 pairs, 2 squarings (1 x 1, 2 x 2), 20 aliased; lr_bfv_mul: 1 x 1, its squaring, 1 aliased)
    assert calls == 3 * 3 * (20 + 2 + 20 + 3) and refusals == 3 * 15, stdout
