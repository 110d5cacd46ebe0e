"""The BFV encryptor's and decryptor's host side (lattigo-fhe-by-go_amd/csrc/lr_bfv_encryptor.cpp: the argument checks, the pools, the staging
through the pinned buffer, the named steps of both shapes) under AddressSanitizer + UBSan and under ThreadSanitizer (CPU build only), driven by
tests/cpp/bfv_encryptor_driver.cpp: pk and sk, fast and through P, host and device-pointer randomness, the default shape and
lr_options::no_epilogue, batches 1, 3 and max_batch with pool and staging reuse across calls, Decrypt at degrees 0, 1, 2 and 9, two handles on
two threads, the recorded launch sequence of both shapes for pk through P (call by call: the reference's call order), and every refusal.  The
stubs touch the first and the last byte of everything a kernel would read or write, so a wrong buffer size, stride or batch count is a
sanitizer report."""
import os
import subprocess

import pytest

from host_stub_build import build_host_driver, expected_refusals, refusal_messages


@pytest.mark.parametrize("tag,flags,env", [
    ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}),
    ("tsan", ["-fsanitize=thread"], {"TSAN_OPTIONS": "halt_on_error=1 second_deadlock_stack=1"}),
])
def test_bfv_encryptor_host_side_under_sanitizers(tmp_path, tag, flags, env):
    exe = build_host_driver(str(tmp_path), "bfv_encryptor_driver", flags, tag, units=["lr_bfv_encryptor"],
                            stubs=["bfv_encryptor_stub"])
    clean = {k: v for k, v in os.environ.items() if not k.startswith("LR_")}       # the handles' options decide the shapes, not the caller's env
    res = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(clean, **env))
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-6000:])
    assert "failures 0" in res.stdout, res.stdout
    assert refusal_messages(res.stdout) == expected_refusals("bfv_encryptor_driver")       # the texts that reach the callers, message for message
    calls = int(res.stdout.split("calls ")[1].split(",")[0])
    refusals = int(res.stdout.split("refusals ")[1].split(",")[0])
    # 6 runs (2 degrees x 2 shapes, and 2 on threads) x 2 rounds x 3 batches x (8 encrypt + 8 decrypt calls); 12 refusals at creation, 40 at the calls
    assert calls == 6 * 2 * 3 * 16 and refusals == 52, res.stdout
