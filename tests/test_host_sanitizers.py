"""Host concurrency of the C ABI under ThreadSanitizer and AddressSanitizer + UBSan (CPU build only; GPU sanitizers are not available on the
pool).  The product's host code -- lattigo-fhe-by-go_amd/csrc/lr_abi_*.cpp, lr_host.hpp, lr_precompute.cpp -- is compiled with g++ against
the host-only HIP stand-in and the recording launch stubs of tests/cpp/hipstub/ and driven by tests/cpp/host_concurrency.cpp: 64 threads
mixing batched MulRelin / rotation requests, refused requests, an injected device failure in the middle of a batch, direct pipelines over
shared contexts, scratch leases, handle churn and peer copies.  A sanitizer report fails the test; so does a caller that got another
caller's result back (the stubs carry one tag word per poly through the pipelines)."""
import os
import subprocess

import pytest

from host_stub_build import build_host_driver


@pytest.mark.parametrize("tag,flags,env", [
    ("tsan", ["-fsanitize=thread"], {"TSAN_OPTIONS": "halt_on_error=1 second_deadlock_stack=1"}),
    ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}),
])
def test_host_concurrency_under_sanitizers(tmp_path, tag, flags, env):
    exe = build_host_driver(str(tmp_path), "host_concurrency", flags, tag)
    # no LR_* override may leak in from the caller's environment: the run is about the default paths
    clean = {k: v for k, v in os.environ.items() if not k.startswith("LR_")}
    res = subprocess.run([exe, "64", "12"], capture_output=True, text=True, timeout=900, env=dict(clean, **env))
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-6000:])
    assert "failures 0" in res.stdout and "callers of the failed batch" in res.stdout, res.stdout
    served = int(res.stdout.split("served ")[1].split(",")[0])
    failed_callers = int(res.stdout.split("callers of the failed batch ")[1].split(",")[0])
    assert served > 100 and failed_callers >= 1, res.stdout             # the injected failure reached at least one caller, and only as an error code
