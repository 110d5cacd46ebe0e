"""Host concurrency of the C ABI under ThreadSanitizer and AddressSanitizer + UBSan (CPU build only; GPU sanitizers are not available on the
pool).  The product's host code -- every lattigo-fhe-by-go_amd/csrc/lr_*.cpp but lr_asm.cpp -- is compiled with g++ against
the host-only HIP stand-in and the recording launch stubs of tests/cpp/hipstub/ and driven by tests/cpp/host_concurrency.cpp: 64 threads
mixing batched MulRelin / rotation requests, refused requests, an injected device failure in the middle of a batch, direct pipelines over
shared contexts, scratch leases, handle churn and peer copies.  A sanitizer report fails the test; so does a caller that got another
caller's result back (the stubs carry one tag word per poly through the pipelines)."""
import pytest

from host_stub_build import SANITIZERS, run_host_driver


@pytest.mark.parametrize("tag,flags,env", SANITIZERS[::-1])
def test_host_concurrency_under_sanitizers(tmp_path, tag, flags, env):
    # (no LR_* override leaks in from the caller's environment: the run is about the default paths)
    stdout, _, _ = run_host_driver(tmp_path, "host_concurrency", tag, flags, env, args=[64, 12])
    assert "callers of the failed batch" in stdout, stdout
    served = int(stdout.split("served ")[1].split(",")[0])
    failed_callers = int(stdout.split("callers of the failed batch ")[1].split(",")[0])
    assert served > 100 and failed_callers >= 1, stdout             # the injected failure reached at least one caller, and only as an error code
