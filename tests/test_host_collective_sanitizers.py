"""The collective handle's host side (lattigo-fhe-by-go_amd/csrc/lr_collective.cpp: the argument checks, the pool, the staging through the
pinned buffer, the rows a call at a level reads, the fold's passes, the named steps of both shapes) under AddressSanitizer + UBSan and under
ThreadSanitizer (CPU build only), driven by the stand-alone program tests/cpp/collective_driver.cpp: every entry point in its host and
device-pointer form, the default shape and lr_options::no_epilogue, batches 1, 3 and max_batch (5) with pool and staging reuse across
consecutive host-form calls, every level, |P| = 1 and |P| = 2, 33 shares (a second fold pass) with out aliasing a share and the base, two
handles on two threads, the launch counts of both shapes, and every refusal.  The stubs touch the first and the last byte of everything a
kernel would read or write, so a wrong buffer size, stride, level or share count is a sanitizer report."""
import pytest

from host_stub_build import SANITIZERS, expected_refusals, refusal_messages, run_host_driver


@pytest.mark.parametrize("tag,flags,env", SANITIZERS)
def test_collective_host_side_under_sanitizers(tmp_path, tag, flags, env):
    stdout, calls, refusals = run_host_driver(tmp_path, "collective_driver", tag, flags, env)
    assert refusal_messages(stdout) == expected_refusals("collective_driver")       # the texts that reach the callers, message for message
    assert stdout.count("launches ") == 2 * (1 + 7), stdout               # the ModDowns and seven calls, in both shapes
    # 8 runs (2 degrees x 2, 2 more at N = 16, and 2 on threads) x 2 rounds x 3 batches x 12 calls (8 share forms, 4 folds);
    # 9 refusals at creation, 69 at the calls
    assert calls == 8 * 2 * 3 * 12 and refusals == 78, stdout
