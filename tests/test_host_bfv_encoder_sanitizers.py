"""The BFV encoder's host side (lattigo-fhe-by-go_amd/csrc/lr_bfv_encoder.cpp: the route decision, the tables, the staging through the pinned
buffer, the named stages of both routes) under AddressSanitizer + UBSan (CPU build only), driven by tests/cpp/bfv_encoder_driver.cpp: both
routes, batches 1, 3 and max_batch, n_values 0, 1 and N, host-value and device-pointer entry points, and every refusal.  The stubs touch the
first and the last word of everything a kernel would read or write, so a wrong buffer size, stride or batch count is a sanitizer report."""
from host_stub_build import ASAN_UBSAN, run_host_driver


def test_bfv_encoder_host_side_under_asan_ubsan(tmp_path):
    stdout, calls, refusals = run_host_driver(tmp_path, "bfv_encoder_driver", *ASAN_UBSAN)
    # 7 encoders (2 degrees x 3 routes, and N = 2^4) x 3 batches x 3 n_values x 8 entry-point calls; 6 refusals at creation and 22 at the calls
    assert calls == 7 * 3 * 3 * 8 and refusals == 28, stdout
