"""The collective setup's host side (lattigo-fhe-by-go_amd/csrc/lr_setup.cpp: the argument checks, the pool, the staging through the pinned
buffer, the passes over chunks of parties, the named steps of both shapes, the fold over all of Q||P) under AddressSanitizer + UBSan and
under ThreadSanitizer (CPU build only), driven by tests/cpp/setup_driver.cpp: every entry point in its host and device-pointer form, the
default shape and lr_options::no_epilogue, 1, 3 and max_batch parties (5, and 70: three passes of at most 32 parties) with pool and
staging reuse across consecutive host-form calls, |P| = 1 and a ragged |P| = 2, two handles on two threads, the launch counts of both
shapes, and every refusal.  The stubs touch the first and the last byte of everything a kernel would read or write, so a wrong buffer
size, stride, digit or party count is a sanitizer report."""
import pytest

from host_stub_build import SANITIZERS, expected_refusals, refusal_messages, run_host_driver


@pytest.mark.parametrize("tag,flags,env", SANITIZERS)
def test_setup_host_side_under_sanitizers(tmp_path, tag, flags, env):
    stdout, calls, refusals = run_host_driver(tmp_path, "setup_driver", tag, flags, env)
    assert refusal_messages(stdout) == expected_refusals("setup_driver")        # the texts that reach the callers, message for message
    # 10 runs (2 degrees x 2, 2 more at N = 16, 2 with 70 parties, and 2 on threads) x 2 rounds x 3 party counts x 20 accepted calls
    # (14 share calls, 3 finalize steps, 3 folds); 9 refusals at creation (the 64-limb LR_ERR_UNSUPPORTED among them), 109 at the calls
    assert calls == 10 * 2 * 3 * 20 and refusals == 118, stdout
