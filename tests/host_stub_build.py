"""The CPU build of the product's host side that the sanitizer tests share: every lattigo-fhe-by-go_amd/csrc/lr_abi_*.cpp, lr_host.hpp and
lr_precompute.cpp, compiled with g++ against the host-only HIP stand-in and the recording launch stubs of tests/cpp/hipstub/ (hipstub.cpp,
stub_launch.cpp: the launchers of both evaluator units, lr_abi_bfv_eval.cpp and lr_abi_ckks_eval.cpp, among them), and linked with one
driver from tests/cpp/.  The handles whose units stay out of the lr_abi_*.cpp set (the encoders, the
encryptors, the key generator, the collective handle) name their unit and the stand-ins of their launchers; the shared set links as it does
without them."""
import concurrent.futures as cf
import glob
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "lattigo-fhe-by-go_amd", "csrc")
STUB = os.path.join(ROOT, "tests", "cpp", "hipstub")


def build_host_driver(tmp, driver, flags, tag, units=(), stubs=()):
    """Compiles the product units (with csrc/<unit>.cpp for each of `units`), tests/cpp/<stub>.cpp for each of `stubs` and
    tests/cpp/<driver>.cpp with `flags` into the directory `tmp`; returns the executable's path."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    srcs = sorted(glob.glob(os.path.join(CSRC, "lr_abi_*.cpp"))) + [os.path.join(CSRC, u + ".cpp") for u in units]
    srcs += [os.path.join(CSRC, "lr_precompute.cpp"), os.path.join(STUB, "hipstub.cpp"), os.path.join(STUB, "stub_launch.cpp")]
    srcs += [os.path.join(cpp, s + ".cpp") for s in stubs] + [os.path.join(cpp, driver + ".cpp")]
    common = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread", "-I" + STUB, "-I" + CSRC, "-I" + os.path.join(ROOT, "include")] + flags

    def one(src):
        obj = os.path.join(tmp, tag + "_" + os.path.basename(src) + ".o")
        subprocess.check_call(common + ["-c", src, "-o", obj])
        return obj
    with cf.ThreadPoolExecutor(max_workers=6) as ex:
        objs = list(ex.map(one, srcs))
    exe = os.path.join(tmp, driver + "_" + tag)
    subprocess.check_call(common + objs + ["-o", exe])
    return exe


def refusal_messages(stdout):
    """the block a driver prints between its two marker lines: one lr_last_error_string() per refused call"""
    return stdout.split("refusal messages begin\n")[1].split("refusal messages end\n")[0]


def expected_refusals(driver):
    with open(os.path.join(ROOT, "tests", "cpp", "expected", driver + "_refusals.txt")) as f:
        return f.read()
