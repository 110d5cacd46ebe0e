"""The transform dispatch (lr_abi_ring.cpp: the route decision ntt_route and the launch switch behind run_ntt), the RNS rescale's plan and stages
and the epilogue-run iterator with its three users, under AddressSanitizer + UBSan (CPU build only).  The product's host code is compiled with
g++ against the host-only HIP stand-in and the recording launch stubs of tests/cpp/hipstub/ (host_stub_build.py) and driven by
tests/cpp/ntt_dispatch_driver.cpp through the public ABI: N = 2^10 .. 2^16, moduli sets for the forward variants 0 .. 3, every option that
changes a route, batches 1 and 3 and one launch that crosses run_ntt's chunking, in place and out of place, and every refusal.  After each
call the driver reads the name of the kernel the context dispatched; the set of names per (ring, moduli, options) is compared with
tests/golden/ntt_dispatch_routes.txt, which was recorded from the dispatcher as it was before it was split into decision and launches.
After those, the modulus classes at the limits of the admission bounds (tests/limit_moduli.py: just under 2^61, either side of 2^57, just
above and just below 2^33) under the options that move them between the assembly variants, the FP64 body and the C++ kernels: the variants
the contexts report must be the ones the Python restatement of the predicates gives, and the kernel names are pinned by the same golden."""
import os

import limit_moduli as lm
from conftest import ROOT
from host_stub_build import ASAN_UBSAN, run_host_driver

# five primes = 1 mod 2^17 per class (NTT-friendly for every ring of the driver)
LIMIT_CLASSES = {"61-": lm.below(61, 16, 5), "57-": lm.below(57, 16, 5), "57+": lm.above(57, 16, 5), "33+": lm.above(33, 16, 5),
                 "33-": lm.below(33, 16, 5)}
LIMIT_OPTIONS = {"default": {}, "no_asm": {"no_asm": True}, "no_fp": {"no_fp": True}, "asm_variant=0": {"asm_variant": 0}, "asm_variant=1": {"asm_variant": 1}}

# one name per route of NttRoute::Kind that a public call can end on ("xK": a plain transform call of K launches; without: the last
# transform of a compound call).  The lazy inverse routes are always followed by another transform inside the call that asks for them, and
# the stamped route needs a diagnostics build: the GPU suite covers those.
ROUTE_WITNESSES = {
    "Cxx": ["ntt_fwd_kernel<10>x1", "ntt_inv_kernel<16>x1"],
    "Whole": ["stub_fwd12_m1x1", "stub_fwd14_m3x1", "stub_inv15_m3x1", "stub_fwd14_m4", "stub_fwd12_m5", "stub_fwd15_m4"],
    "Split15Top": ["stub_fwd15h_m3x2", "stub_fwd15h_m0x2"],
    "Split15Pretop": ["stub_fwd15h_m4", "stub_fwd15h_m5"],
    "Split15InvTop": ["stub_inv15h_m3x2"],
    "Fwd16Pretop": ["stub_fwd16p_m4", "stub_fwd16p_m5"],
    "Fwd16Fused": ["stub_fwd16s_m3x1", "stub_fwd16s_m4", "stub_fwd16s_m5"],
    "Fwd16Top": ["stub_fwd16p_m3x2", "stub_fwd16p_m3x4"],
    "Inv16PairFlags": ["stub_inv16f_m3x1", "stub_inv16f_m3x2"],
    "Inv16Top": ["stub_inv16s_m3x2"],
}


def test_ntt_dispatch_host_side_under_asan_ubsan(tmp_path):
    args = [str(a) for name, qs in LIMIT_CLASSES.items() for a in [name] + qs]
    stdout, calls, refusals = run_host_driver(tmp_path, "ntt_dispatch_driver", *ASAN_UBSAN, args=args, timeout=1500)
    # 5 rings x 4 moduli sets x 10 option sets, one more option set at N = 2^14 and three more at N = 2^15
    # ... and the five limit classes x 5 rings x 5 option sets
    configs = 4 * (5 * 10 + 1 + 3) + len(LIMIT_CLASSES) * 5 * len(LIMIT_OPTIONS)
    # per batch (1 and 3): 18 + 10 transforms, 4 x 5 + 2 x 5 divisions, 3 x 3 rescales of a ciphertext, 3 x 3 ModDowns, 4 x 3 monomial products,
    # 3 x 4 permutations, 2 key switches; the six host-slice transforms at batch 1 only; the three calls of the chunked launch once
    assert calls == configs * (2 * (28 + 30 + 9 + 9 + 12 + 12 + 2) + 6) + 3, stdout[-300:]
    assert refusals == configs * REFUSALS_PER_CONFIG, stdout[-300:]
    got = [ln for ln in stdout.splitlines() if ln.startswith("routes ")]
    want = open(os.path.join(ROOT, "tests", "golden", "ntt_dispatch_routes.txt")).read().splitlines()
    assert len(got) == configs
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
    # the limit classes: what the contexts report is what the restated predicates say (a changed bound shows here, next to the golden)
    seen = 0
    for ln in got:
        head = ln.split(":", 1)[0].split()
        cls, opt = head[2].split("=", 1)[1], head[3]
        if cls in LIMIT_CLASSES:
            want_fwd, want_inv = lm.asm_variants(LIMIT_CLASSES[cls], **LIMIT_OPTIONS[opt])
            assert head[4:] == ["fwd=%d" % want_fwd, "inv=%d" % want_inv], ln
            seen += 1
    assert seen == len(LIMIT_CLASSES) * 5 * len(LIMIT_OPTIONS)
    names = {n for ln in got for n in ln.split(":", 1)[1].split()}
    for route, witnesses in ROUTE_WITNESSES.items():
        for w in witnesses:
            assert w in names, (route, w)


# lr_ntt / lr_intt 9 each, lr_ntt_limb / lr_intt_limb 8 each, lr_ntt_host / lr_intt_host 5 each, lr_ntt_host_limb 4, the four single divisions 4 each,
# the two ...Many 4 in either domain, lr_ckks_rescale 3, the ModDowns 4, lr_mult_by_monomial 4, lr_shift 5, lr_permute 4, lr_permute_ntt 4
REFUSALS_PER_CONFIG = 2 * 9 + 2 * 8 + 2 * 5 + 4 + 4 * 4 + 2 * 2 * 4 + 3 + 4 + 4 + 5 + 4 + 4
