"""The CKKS power basis' host side (lattigo-fhe-by-go_amd/csrc/lr_abi_ckks_scalar.cpp and lr_abi_ckks_eval.cpp: the schedule's recursion and scalar lines, the argument
and shape checks in the header's order, the route decision, the grouping into layers and chunks, the pointer tables and words in their
pinned slots, the staging pair and its divisions, the views the composed route rescales) under AddressSanitizer + UBSan and under
ThreadSanitizer (CPU build only, each run as its own executable), driven by tests/cpp/ckks_basis_driver.cpp: both routes, four degrees,
two option sets, three max_batch values, ten schedules, outputs of exactly level_after + 1 limbs, first calls on fresh plans, the launch
counts of each route, two plans on two threads, and every refusal.  The stand-in of its launcher (tests/cpp/hipstub/stub_launch.cpp)
touches the first and the last word of every row and table entry the kernel would read or write, so a wrong pool size, stride, level or
table offset is a sanitizer report."""
import pytest

from host_stub_build import SANITIZERS, number, run_host_driver


@pytest.mark.parametrize("tag,flags,env", SANITIZERS)
def test_ckks_basis_host_side_under_sanitizers(tmp_path, tag, flags, env):
    stdout, calls, refusals = run_host_driver(tmp_path, "ckks_basis_driver", tag, flags, env)
    # per ring and option set: 3 max_batch values x (10 schedules + 1 at batch 1) x 2 output sizes, 2 calls at batch 8, the accepted call among the
    # refusals, 3 first calls x 2 x 2; on the merged route (3 rings, default options) the MulRelin calls and the call of the launch
    # count: 3 + 2 + 2 chunks and one call per max_batch; 2 threads x 10 schedules x 2
    assert calls == 4 * 2 * (3 * 11 * 2 + 2 + 1 + 3 * 2 * 2) + 3 * (3 + 2 + 2 + 3) + 2 * 10 * 2, stdout
    assert refusals == 4 * 2 * 52, stdout
    assert number(stdout, "tail launches") > 0 and number(stdout, "combine launches") > 0, stdout
    assert number(stdout, "tail products") > number(stdout, "tail launches"), stdout           # chunks of more than one product ran
