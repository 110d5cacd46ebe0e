"""The CPU build of the product's host side that the sanitizer tests share.  One rule names the product set: every
lattigo-fhe-by-go_amd/csrc/lr_*.cpp except lr_asm.cpp, whose launchers tests/cpp/hipstub/stub_launch.cpp stands in for.  It is compiled with
g++ against the host-only HIP stand-in and every launch stand-in of tests/cpp/hipstub/, once per flag set and pytest process, and linked
with one driver from tests/cpp/ per test.  run_host_driver is what a test calls; its own assertions are all that is left to it."""
import atexit
import concurrent.futures as cf
import glob
import os
import shutil
import subprocess
import tempfile

from conftest import ROOT

CSRC = os.path.join(ROOT, "lattigo-fhe-by-go_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")
STUB = os.path.join(CPP, "hipstub")

# (tag, flags, env) of the two sanitizer configurations: a test's parametrisation, or the arguments of one run
ASAN_UBSAN = ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
              {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
TSAN = ("tsan", ["-fsanitize=thread"], {"TSAN_OPTIONS": "halt_on_error=1 second_deadlock_stack=1"})
SANITIZERS = [ASAN_UBSAN, TSAN]

_product_objects = {}       # flag tuple -> the objects of the product set and the stand-ins, in a directory that goes at exit


def _compiler(flags):
    return ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread", "-I" + STUB, "-I" + CSRC,
            "-I" + os.path.join(ROOT, "include")] + list(flags)


def _compile(flags, src, obj):
    subprocess.check_call(_compiler(flags) + ["-c", src, "-o", obj])
    return obj


def product_objects(flags):
    key = tuple(flags)
    if key not in _product_objects:
        srcs = [s for s in sorted(glob.glob(os.path.join(CSRC, "lr_*.cpp"))) if os.path.basename(s) != "lr_asm.cpp"]
        srcs += sorted(glob.glob(os.path.join(STUB, "*.cpp")))
        out = tempfile.mkdtemp(prefix="lr_host_objects_")
        atexit.register(shutil.rmtree, out, ignore_errors=True)
        with cf.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
            _product_objects[key] = list(ex.map(lambda s: _compile(flags, s, os.path.join(out, os.path.basename(s) + ".o")), srcs))
    return _product_objects[key]


def build_host_driver(tmp, driver, flags, tag):
    """Compiles tests/cpp/<driver>.cpp with `flags` and links it with the product set built with the same flags; returns the path of the
    executable, which lies in the directory `tmp`."""
    obj = _compile(flags, os.path.join(CPP, driver + ".cpp"), os.path.join(tmp, driver + "_" + tag + ".o"))
    exe = os.path.join(tmp, driver + "_" + tag)
    subprocess.check_call(_compiler(flags) + [obj] + product_objects(flags) + ["-o", exe])
    return exe


def number(stdout, what):
    """the figure behind the first "<what> " of a driver's output, None where it prints none"""
    return int(stdout.split(what + " ")[1].split(",")[0]) if what + " " in stdout else None


def run_host_driver(tmp, driver, tag, flags, env, args=(), timeout=900, summary=True):
    """Builds the driver and runs it with `args`, under `env` and without the caller's LR_* variables (the handles' options decide the
    paths, not the environment).  The run must exit with 0 and, where the driver prints a summary line, report no failure.  Returns its
    stdout and the calls and refusals of the summary line."""
    exe = build_host_driver(str(tmp), driver, flags, tag)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("LR_")}
    res = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, env=dict(clean, **env))
    print(res.stdout[-3000:])
    assert res.returncode == 0, (res.stdout[-3000:], res.stderr[-6000:])
    if summary:
        assert "failures 0" in res.stdout, res.stdout[-3000:]
    return res.stdout, number(res.stdout, "calls"), number(res.stdout, "refusals")


def refusal_messages(stdout):
    """the block a driver prints between its two marker lines: one lr_last_error_string() per refused call"""
    return stdout.split("refusal messages begin\n")[1].split("refusal messages end\n")[0]


def expected_refusals(driver):
    with open(os.path.join(CPP, "expected", driver + "_refusals.txt")) as f:
        return f.read()
