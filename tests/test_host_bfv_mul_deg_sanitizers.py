"""lr_bfv_mul_deg's host side under AddressSanitizer + UBSan (CPU build only).  The product's host code -- every lattigo-fhe-by-go_amd/csrc/
lr_abi_*.cpp, lr_bfv_tensor.cpp (the unit of lr_bfv_mul_deg), lr_host.hpp, lr_precompute.cpp -- is compiled with g++ against the host-only HIP
stand-in and the recording launch stubs of tests/cpp/hipstub/ (stub_launch.cpp, and stub_tensor_deg.cpp for the general-degree tensor), and
driven by tests/cpp/bfv_mul_deg_driver.cpp: every degree pair, the squaring case, batches on both sides of the gather threshold, the paths
without gathering and without the extension epilogues, aliased outputs and every refusal.  The stubs touch the first and the last word of
every row a kernel would read or write, so a wrong pool size, slot offset or stride is a sanitizer report."""
import concurrent.futures as cf
import glob
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "lattigo-fhe-by-go_amd", "csrc")
STUB = os.path.join(ROOT, "tests", "cpp", "hipstub")


def test_bfv_mul_deg_host_side_under_asan_ubsan(tmp_path):
    units = sorted(glob.glob(os.path.join(CSRC, "lr_abi_*.cpp"))) + [
        os.path.join(CSRC, "lr_bfv_tensor.cpp"), os.path.join(CSRC, "lr_precompute.cpp"), os.path.join(STUB, "hipstub.cpp"),
        os.path.join(STUB, "stub_launch.cpp"), os.path.join(STUB, "stub_tensor_deg.cpp"), os.path.join(ROOT, "tests", "cpp", "bfv_mul_deg_driver.cpp")]
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    common = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread", "-I" + STUB, "-I" + CSRC,
              "-I" + os.path.join(ROOT, "include")] + flags

    def one(src):
        obj = os.path.join(str(tmp_path), os.path.basename(src) + ".o")
        subprocess.check_call(common + ["-c", src, "-o", obj])
        return obj
    with cf.ThreadPoolExecutor(max_workers=6) as ex:
        objs = list(ex.map(one, units))
    exe = os.path.join(str(tmp_path), "bfv_mul_deg_driver")
    subprocess.check_call(common + objs + ["-o", exe])
    clean = {k: v for k, v in os.environ.items() if not k.startswith("LR_")}       # the plans' options decide the paths, not the caller's env
    env = dict(clean, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-6000:])
    assert "failures 0" in res.stdout, res.stdout
    calls = int(res.stdout.split("calls ")[1].split(",")[0])
    refusals = int(res.stdout.split("refusals ")[1].split(",")[0])
    assert calls == 3 * 3 * (20 + 2 + 20) and refusals == 3 * 14, res.stdout      # 3 plans x 3 batches x (20 pairs, 2 squarings, 20 aliased)
