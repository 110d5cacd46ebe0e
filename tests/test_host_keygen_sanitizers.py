"""The key generator's host side (lattigo-fhe-by-go_amd/csrc/lr_keygen.cpp: the argument checks, the pool, the staging through the pinned
buffer, the passes over chunks of keys, the named steps of both shapes) under AddressSanitizer + UBSan and under ThreadSanitizer (CPU build
only), driven by tests/cpp/keygen_driver.cpp: every entry point in its host and device-pointer form, the default shape and
lr_options::no_epilogue, 1, 3 and max_batch keys (5, and 70: three passes of at most 32 keys) with pool and staging reuse across consecutive host-form calls, |P| = 1 and a ragged
|P| = 2, two handles on two threads, the launch counts of both shapes, and every refusal.  The stubs touch the first and the last byte of
everything a kernel would read or write, so a wrong buffer size, stride, digit or key count is a sanitizer report."""
import pytest

from host_stub_build import SANITIZERS, expected_refusals, refusal_messages, run_host_driver


@pytest.mark.parametrize("tag,flags,env", SANITIZERS)
def test_keygen_host_side_under_sanitizers(tmp_path, tag, flags, env):
    stdout, calls, refusals = run_host_driver(tmp_path, "keygen_driver", tag, flags, env)
    assert refusal_messages(stdout) == expected_refusals("keygen_driver")       # the texts that reach the callers, message for message
    # 10 runs (2 degrees x 2, 2 more at N = 16, 2 with 70 keys, and 2 on threads) x 2 rounds x 3 key counts x 5 entry points x 2 forms;
    # 8 refusals at creation, 58 at the calls
    assert calls == 10 * 2 * 3 * 10 and refusals == 66, stdout
