"""lr_bfv_relinearize_deg's host side (lattigo-fhe-by-go_amd/csrc/lr_abi_bfv_eval.cpp: the argument and shape checks in the header's order, the
route decision, the passes of G groups, the gather, the grouped key switch's member ranges in lr_abi_ckks.cpp, the fold's operands) under
AddressSanitizer + UBSan and under ThreadSanitizer (CPU build only, each run as its own executable), driven by
tests/cpp/bfv_relin_deg_driver.cpp: both routes, degrees 1 to 5, batches 1, 2 and max_batch with max_batch 4 and 3 (G = 1, partial and
full), every aliasing the header allows, first calls on fresh plans, the launch counts of each route, two plans on two threads, and every
refusal.  The stand-in of the new launcher touches the first and the last word of every row the kernel would read or write, so a wrong
pool size, stride or group distance is a sanitizer report."""
import pytest

from host_stub_build import SANITIZERS, run_host_driver


@pytest.mark.parametrize("tag,flags,env", SANITIZERS)
def test_bfv_relin_deg_host_side_under_sanitizers(tmp_path, tag, flags, env):
    stdout, calls, refusals = run_host_driver(tmp_path, "bfv_relin_deg_driver", tag, flags, env)
    folds = int(stdout.split("fold launches ")[1].split(",")[0])
    # per batch: 5 degrees x 6 calls and one more from degree 3 on; per plan: 3 batches, 2 calls among the refusals, 5 x 2 first calls
    per_batch = 5 * 6 + 3
    assert calls == 3 * 3 * 2 * (3 * per_batch + 2 + 10) + 2 * 2 * per_batch, stdout
    assert refusals == 3 * 3 * 2 * 39 and folds > 0, stdout
