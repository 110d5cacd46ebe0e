"""The CKKS rotation chain's host side (lattigo-fhe-by-go_amd/csrc/lr_abi_ckks_eval.cpp: the argument and shape checks in the header's order,
the route decision, the two pool pairs that state and destination alternate on, the copy for crossed outputs, the second stride of the
key switch's last pass, the detour of a one-step accumulating chain in place) under AddressSanitizer + UBSan and under ThreadSanitizer
(CPU build only, each run as its own executable), driven by tests/cpp/ckks_chain_driver.cpp: lr_ckks_rotate_chain on both routes, four
degrees, three option sets, levels 0, 2 and the top, batches 1, 2 and max_batch, every aliasing the header allows and polys of three
different strides, first calls on fresh plans, the launch counts of each route, two plans on two threads, and every refusal.  The stand-in
of its launcher (tests/cpp/hipstub/stub_launch.cpp) touches the first and the last word of every row the kernel would read or write, so a
wrong pool size, stride or level is a sanitizer report."""
import pytest

from host_stub_build import SANITIZERS, run_host_driver


@pytest.mark.parametrize("tag,flags,env", SANITIZERS)
def test_ckks_chain_host_side_under_sanitizers(tmp_path, tag, flags, env):
    stdout, calls, refusals = run_host_driver(tmp_path, "ckks_chain_driver", tag, flags, env)
    steps = int(stdout.split("step launches ")[1].split(",")[0])
    # 4 degrees x 3 option sets x (3 levels x 3 batches x 48 calls + 1 accepted call among the refusals + 6 first calls) and
    # 2 threads x 2 batches x 48 calls
    assert calls == 4 * 3 * (3 * 3 * 48 + 1 + 6) + 2 * 2 * 48, stdout
    assert refusals == 4 * 3 * 24, stdout
    # the fused route (accumulating chains; three degrees, two option sets): per level and batch 6 aliasings x (0 + 1 + 2 + 3) steps, the
    # accepted call's 2 and the first calls' 2 x (3 + 1); and the thread at N = 2^12
    assert steps == 3 * 2 * (3 * 3 * 6 * 6 + 2 + 2 * 4) + 2 * 6 * 6, stdout
