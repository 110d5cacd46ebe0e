"""The Refresh handle's host side (lattigo-fhe-by-go_amd/csrc/lr_refresh.cpp: the argument checks, the pool, the staging of mask and noise
through the pinned buffer, the word counts and Recode's tables per levelStart, the rows each step reads, the fold's passes, the steps of both
shapes) under AddressSanitizer + UBSan and under ThreadSanitizer (CPU build only), driven by the stand-alone program
tests/cpp/refresh_driver.cpp: every entry point in its host and device-pointer form, the default shape and lr_options::no_epilogue,
batches 1, 3 and max_batch (5) with pool and staging reuse across consecutive host-form calls, every levelStart, ctxP present (|P| = 1
and 2) and absent, 33 shares (a second fold pass) with out aliasing a share, two handles on two threads, and every refusal.  The stubs
touch the first and the last byte of everything a kernel would read or write, so a wrong buffer size, stride, level or word count is a
sanitizer report."""
import pytest

from host_stub_build import SANITIZERS, expected_refusals, refusal_messages, run_host_driver


@pytest.mark.parametrize("tag,flags,env", SANITIZERS)
def test_refresh_host_side_under_sanitizers(tmp_path, tag, flags, env):
    stdout, calls, refusals = run_host_driver(tmp_path, "refresh_driver", tag, flags, env)
    assert refusal_messages(stdout) == expected_refusals("refresh_driver")          # the texts that reach the callers, message for message
    # per run 2 rounds x 3 batches x (3 levelStarts x 6 CKKS calls + 4 folds [+ 4 BFV calls with a ctxP]): 156 with a ctxP, 132 without;
    # 8 runs with a ctxP (2 degrees x 2, 2 more at N = 16, 2 on threads) and 2 without; 9 refusals at creation, 101 at the calls
    assert calls == 8 * 156 + 2 * 132 and refusals == 110, stdout
