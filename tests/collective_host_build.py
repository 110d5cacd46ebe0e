"""The CPU build of the collective handle's host side for its sanitizer test: what host_stub_build.py compiles (every lr_abi_*.cpp,
lr_precompute.cpp, the host-only HIP stand-in and its launch stubs, all unchanged) plus lattigo-fhe-by-go_amd/csrc/lr_collective.cpp and the
stand-ins for its launchers: tests/cpp/ckks_encryptor_stub.cpp and tests/cpp/bfv_encryptor_stub.cpp for the expansions and the pk pass it
shares with the encryptors, tests/cpp/collective_stub.cpp for its own.  The unit stays out of the lr_abi_*.cpp set, so the shared build
and the sanitizer tests on it link as before."""
import concurrent.futures as cf
import glob
import os
import subprocess

from host_stub_build import CSRC, ROOT, STUB


def build_collective_driver(tmp, driver, flags, tag):
    """Compiles the product units and tests/cpp/<driver>.cpp with `flags` into the directory `tmp`; returns the executable's path."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    units = sorted(glob.glob(os.path.join(CSRC, "lr_abi_*.cpp"))) + [os.path.join(CSRC, "lr_collective.cpp"), os.path.join(CSRC, "lr_precompute.cpp"),
                                                                      os.path.join(STUB, "hipstub.cpp"), os.path.join(STUB, "stub_launch.cpp"),
                                                                      os.path.join(cpp, "bfv_encryptor_stub.cpp"), os.path.join(cpp, "ckks_encryptor_stub.cpp"),
                                                                      os.path.join(cpp, "collective_stub.cpp"), os.path.join(cpp, driver + ".cpp")]
    common = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread", "-I" + STUB, "-I" + CSRC, "-I" + os.path.join(ROOT, "include")] + flags

    def one(src):
        obj = os.path.join(tmp, tag + "_" + os.path.basename(src) + ".o")
        subprocess.check_call(common + ["-c", src, "-o", obj])
        return obj
    with cf.ThreadPoolExecutor(max_workers=6) as ex:
        objs = list(ex.map(one, units))
    exe = os.path.join(tmp, driver + "_" + tag)
    subprocess.check_call(common + objs + ["-o", exe])
    return exe
