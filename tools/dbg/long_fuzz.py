"""One-off extended fuzz on the GPU box: the bodies of tests/test_gpu_fuzz.py and tests/test_gpu_handle_fuzz.py with seeds far beyond the
committed ranges.
    python tools/dbg/long_fuzz.py [first_seed] [count] [--families ring|handles|all|name,name,...]
A mismatch (AssertionError) is counted and the run goes on to the next seed.  Anything else -- a HIP error, a refusal, an abort -- ends the
run at once with a non-zero status: nothing more is started on a device that may have faulted."""
import argparse
import os
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import test_gpu_fuzz as F  # noqa: E402
import test_gpu_handle_fuzz as H  # noqa: E402

RING = {name[len("test_"):-len("_fuzz")]: getattr(F, name) for name in (
    "test_ntt_and_elementwise_fuzz", "test_basis_extension_and_rescale_fuzz", "test_key_switch_fuzz", "test_dual_kernel_fuzz", "test_mulrelin_rescale_fuzz",
    "test_rotation_encrypt_decrypt_fuzz", "test_moddown_divfloor_permute_fuzz", "test_bfv_pipelines_fuzz")}
HANDLES = dict(H.BODIES)

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("first", nargs="?", type=int, default=100)
ap.add_argument("count", nargs="?", type=int, default=200)
ap.add_argument("--families", default="ring", help="ring (the default), handles, all, or names separated by commas")
opts = ap.parse_args()
known = dict(RING, **HANDLES)
bodies = {"ring": RING, "handles": HANDLES, "all": known}.get(opts.families)
if bodies is None:
    unknown = [n for n in opts.families.split(",") if n not in known]
    if unknown:
        sys.exit("unknown families %s; known: %s" % (unknown, ", ".join(known)))
    bodies = {n: known[n] for n in opts.families.split(",")}
first, count = opts.first, opts.count

pkg, oracle = g.load_package(), g.load_oracle()
fails = 0
t0 = time.time()
for name, fn in bodies.items():
    done = 0
    for seed in range(first, first + count):
        try:
            fn(pkg, oracle, seed)
            done += 1
        except AssertionError:                                           # a mismatch: counted, and the next seed runs
            fails += 1
            print("FAIL", name, seed)
            traceback.print_exc(limit=3)
        except BaseException:                                            # anything else may be a faulted device: stop here
            print("STOP", name, seed, "after %d seeds ok" % done, flush=True)
            traceback.print_exc()
            sys.stdout.flush()
            os._exit(2)
    print("%s: %d of %d seeds ok, seeds %d .. %d (%.0f s)" % (name, done, count, first, first + count - 1, time.time() - t0), flush=True)
print("failures:", fails)
sys.exit(1 if fails else 0)
