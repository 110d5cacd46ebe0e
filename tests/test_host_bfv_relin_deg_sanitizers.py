"""lr_bfv_relinearize_deg's host side (lattigo-fhe-by-go_amd/csrc/lr_abi_bfv_eval.cpp: the argument and shape checks in the header's order, the
route decision, the passes of G groups, the gather, the grouped key switch's member ranges in lr_abi_ckks.cpp, the fold's operands) under
AddressSanitizer + UBSan and under ThreadSanitizer (CPU build only, each run as its own executable), driven by
tests/cpp/bfv_relin_deg_driver.cpp: both routes, degrees 1 to 5, batches 1, 2 and max_batch with max_batch 4 and 3 (G = 1, partial and
full), every aliasing the header allows, first calls on fresh plans, the launch counts of each route, two plans on two threads, and every
refusal.  The stand-in of the new launcher touches the first and the last word of every row the kernel would read or write, so a wrong
pool size, stride or group distance is a sanitizer report."""
import os
import subprocess

import pytest

from host_stub_build import build_host_driver


@pytest.mark.parametrize("tag,flags,env", [
    ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}),
    ("tsan", ["-fsanitize=thread"], {"TSAN_OPTIONS": "halt_on_error=1 second_deadlock_stack=1"}),
])
def test_bfv_relin_deg_host_side_under_sanitizers(tmp_path, tag, flags, env):
    exe = build_host_driver(str(tmp_path), "bfv_relin_deg_driver", flags, tag)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("LR_")}       # the plans' options decide the routes, not the caller's env
    res = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(clean, **env))
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-6000:])
    assert "failures 0" in res.stdout, res.stdout
    calls = int(res.stdout.split("calls ")[1].split(",")[0])
    refusals = int(res.stdout.split("refusals ")[1].split(",")[0])
    folds = int(res.stdout.split("fold launches ")[1].split(",")[0])
    # per batch: 5 degrees x 6 calls and one more from degree 3 on; per plan: 3 batches, 2 calls among the refusals, 5 x 2 first calls
    per_batch = 5 * 6 + 3
    assert calls == 3 * 3 * 2 * (3 * per_batch + 2 + 10) + 2 * 2 * per_batch, res.stdout
    assert refusals == 3 * 3 * 2 * 39 and folds > 0, res.stdout
