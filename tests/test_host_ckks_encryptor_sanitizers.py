"""The CKKS encryptor's host side (lattigo-fhe-by-go_amd/csrc/lr_ckks_encryptor.cpp: the argument checks, the pools, the staging through the
pinned buffer, the named steps of both shapes) under AddressSanitizer + UBSan and under ThreadSanitizer (CPU build only), driven by
tests/cpp/ckks_encryptor_driver.cpp: pk and sk, fast and through P, the top level and level 0, host and device-pointer randomness, the default
shape and lr_options::no_epilogue, batches 1, 3 and max_batch with pool and staging reuse across consecutive host-form calls, two handles on
two threads, the launch counts of the fast forms in both shapes, and every refusal.  The stubs touch the first and the last byte of
everything a kernel would read or write, so a wrong buffer size, stride or batch count is a sanitizer report."""
import pytest

from host_stub_build import SANITIZERS, expected_refusals, refusal_messages, run_host_driver


@pytest.mark.parametrize("tag,flags,env", SANITIZERS)
def test_ckks_encryptor_host_side_under_sanitizers(tmp_path, tag, flags, env):
    stdout, calls, refusals = run_host_driver(tmp_path, "ckks_encryptor_driver", tag, flags, env)
    assert refusal_messages(stdout) == expected_refusals("ckks_encryptor_driver")       # the texts that reach the callers, message for message
    # 6 runs (2 degrees x 2 shapes, and 2 on threads) x 2 rounds x 3 batches x 2 forms x 2 levels x 4 entry points; 8 refusals at creation, 33 at the calls
    assert calls == 6 * 2 * 3 * 16 and refusals == 41, stdout
