// The transform dispatch and the RNS rescale's host side under AddressSanitizer + UBSan (tests/test_host_ntt_dispatch_sanitizers.py): the REAL host
// code -- lr_abi_ring.cpp's route decision (ntt_route), its launch switch (run_ntt) and the rescale's plan and stages, the epilogue-run iterator of
// lr_host.hpp with its three users -- compiled with g++ against the host-only HIP stand-in and the recording launch stubs of tests/cpp/hipstub/.
// Through the public ABI only: lr_ntt, lr_intt, lr_ntt_limb, lr_intt_limb, lr_ntt_host, lr_intt_host, lr_ntt_host_limb, the six
// lr_div_*_by_last_modulus* entry points, lr_ckks_rescale, lr_moddown_ntt_pq, lr_moddown_split_ntt_pq, lr_mult_by_monomial, lr_shift, lr_permute,
// lr_permute_ntt, and one lr_ckks_switch_keys (the producer of the pre-applied top stage) over
//   * N = 2^10 (C++ kernels), 2^12, 2^14, 2^15 and 2^16;
//   * four sets of five moduli, all congruent to 1 modulo 2^17: 45- and 55-bit primes interleaved (forward variant 3, the dual kernels: with
//     no_int_epilogue the epilogue-run iterator yields five runs), 60-bit (variant 1), 61- and 60-bit (variant 0), 55-bit (variant 2);
//   * the options default, no_asm, no_epilogue, no_int_epilogue, rescale_unfused, no_invfuse, no_invtop, no_grid_padding, asm_variant 0 and 1;
//     at N = 2^14 wide14_max_items = 4 (launches of 1, 3, 5 and 15 transforms: both sides of it and of the default 256 never), at N = 2^15
//     ntt_split15 = 0 and 1 and split15_max_workgroups = 4 (both sides, as the default 128 has launches of 1 .. 15 workgroups on one side only);
//   * batches 1 and 3, in place and out of place, rows of one poly into other rows of the same poly (at N = 2^16: the fused top stage; in place:
//     the top pass and the plain sub-blocks; the pre-applied top stage comes from the key switch), every level of the rescale;
//   * once, at N = 2^16: a single-limb launch of 65536 polys, which crosses run_ntt's chunking (65535 / count polys per launch), on memory
//     that is reserved but only touched at the first and the last word of each row;
//   * each entry point's refusals: the code, and that nothing was launched;
//   * after all of that, the modulus classes given on the command line ("name q0 q1 q2 q3 q4", any number of them: the test passes the classes
//     at the limits of the admission bounds -- just under 2^61, either side of 2^57, just above and just below 2^33) on every ring under the
//     options default, no_asm, no_fp, asm_variant 0 and 1: which kernel each limit set selects, pinned without a device.
// After every call the driver reads lr_context_last_ntt_kernel; a plain transform's name carries the number of launches of the call ("x2": a
// streaming top-stage pass beside the sub-block kernels).  One line per (ring, moduli, options) lists the set; the test compares the lines
// with tests/golden/ntt_dispatch_routes.txt.  Routes the stand-in cannot reach (the GPU suite covers them): the stamped whole-transform
// kernels (ntt_timeline) and the persistent forward kernels (ntt_persist), both behind LR_BUILD_DIAG.  The lazy inverse routes (the rounding
// rescale at N = 2^15, the key switch at N = 2^15 / 2^16) are taken, but another transform always follows inside the same public call, so
// no line names them.
// Exit code 0 = every check held; a sanitizer report aborts the run.  Nothing here computes: parity is the GPU suite's business.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include <sys/mman.h>

// a call that went through: ran() below
#define RUN(x) do { const unsigned long long b_ = lr::g_stub_launches.load(); ran(C, (x), b_, false); } while (0)
#define NTT(x) do { const unsigned long long b_ = lr::g_stub_launches.load(); ran(C, (x), b_, true); } while (0)
#include "driver_check.hpp"

static const uint64_t Q60[5] = {1152921504606584833ull, 1152921504598720513ull, 1152921504592429057ull, 1152921504581419009ull, 1152921504580894721ull};
static const uint64_t Q61[2] = {1152921504614055937ull, 1152921504615628801ull};
static const uint64_t Q55[5] = {36028797019488257ull, 36028797023420417ull, 36028797024206849ull, 36028797025124353ull, 36028797032202241ull};
static const uint64_t Q45[3] = {35184372744193ull, 35184373006337ull, 35184376545281ull};
static const int NQ = 5, NP = 2, MAXB = 3;
struct Moduli {
    const char *name;
    uint64_t q[NQ];
    int fwd;            // the forward variant lr_context_ntt_variants reports under the default options
};
static const Moduli kModuli[4] = {{"45/55", {Q45[0], Q55[0], Q45[1], Q55[1], Q45[2]}, 3},
                                  {"60", {Q60[0], Q60[1], Q60[2], Q60[3], Q60[4]}, 1},
                                  {"61/60", {Q61[0], Q60[0], Q60[1], Q61[1], Q60[2]}, 0},
                                  {"55", {Q55[0], Q55[1], Q55[2], Q55[3], Q55[4]}, 2}};
static const uint64_t P[NP] = {36028797033644033ull, 36028797037576193ull};       // (the next two 55-bit primes, in none of the sets)
static const int kLogN[5] = {10, 12, 14, 15, 16};

static const char *set_option(lr_options *o, int v, int logn) {
    switch (v) {
    case 0: return "default";
    case 1: o->no_asm = 1; return "no_asm";
    case 2: o->no_epilogue = 1; return "no_epilogue";
    case 3: o->no_int_epilogue = 1; return "no_int_epilogue";
    case 4: o->rescale_unfused = 1; return "rescale_unfused";
    case 5: o->no_invfuse = 1; return "no_invfuse";
    case 6: o->no_invtop = 1; return "no_invtop";
    case 7: o->no_grid_padding = 1; return "no_grid_padding";
    case 8: o->asm_variant = 0; return "asm_variant=0";
    case 9: o->asm_variant = 1; return "asm_variant=1";
    case 10:
        if (logn == 14) { o->wide14_max_items = 4; return "wide14_max_items=4"; }
        if (logn == 15) { o->ntt_split15 = 0; return "ntt_split15=0"; }
        return nullptr;
    case 11: if (logn == 15) { o->ntt_split15 = 1; return "ntt_split15=1"; } return nullptr;
    case 12: if (logn == 15) { o->split15_max_workgroups = 4; return "split15_max_workgroups=4"; } return nullptr;
    case 13: o->no_fp = 1; return "no_fp";
    default: return nullptr;
    }
}

struct Config {
    uint64_t N;
    lr_context *q = nullptr, *p = nullptr;
    lr_bext *bx = nullptr;
    lr_ckks_plan *pl = nullptr;
    std::set<std::string> names;
};

// the call went through and launched something; what the context says it dispatched joins the configuration's set
static void ran(Config &C, int rc, unsigned long long before, bool plain_transform) {
    CHECK(rc == LR_OK);
    const unsigned long long launches = lr::g_stub_launches.load() - before;
    CHECK(launches > 0);
    ++g_calls;
    char buf[64] = "";
    OK(lr_context_last_ntt_kernel(C.q, buf, sizeof buf));
    std::string s(buf);
    if (s.empty()) return;
    if (plain_transform) s += "x" + std::to_string(launches);
    C.names.insert(s);
}

static void transforms(Config &C, int batch) {
    lr_context *q = C.q;
    lr_poly *a = poly(q, NQ, batch), *b = poly(q, NQ, batch), *wide = poly(q, NQ + 1, batch);
    for (int level : {0, 2, NQ - 1}) {
        NTT(lr_ntt(q, level, a, a));
        NTT(lr_ntt(q, level, a, b));
        NTT(lr_ntt(q, level, a, wide));               // another poly stride
        NTT(lr_intt(q, level, a, a));
        NTT(lr_intt(q, level, b, a));
        NTT(lr_intt(q, level, wide, a));
    }
    for (int inverse = 0; inverse < 2; ++inverse) {
        auto limb = inverse ? lr_intt_limb : lr_ntt_limb;
        NTT(limb(q, 0, a, 0, a, 0));                  // in place
        NTT(limb(q, 1, a, 0, b, 1));
        NTT(limb(q, NQ - 1, a, NQ - 1, a, 0));        // a row of a poly into another row of the same poly
        NTT(limb(q, 2, a, 1, a, 3));
        NTT(limb(q, 3, wide, NQ, a, 3));
    }
    if (batch == 1) {
        std::vector<uint64_t> h((size_t)NQ * C.N, 1);
        const uint64_t *in[NQ];
        uint64_t *out[NQ];
        for (int i = 0; i < NQ; ++i) in[i] = out[i] = h.data() + (size_t)i * C.N;
        for (int level : {0, NQ - 1}) {
            NTT(lr_ntt_host(q, level, in, out));
            NTT(lr_intt_host(q, level, in, out));
        }
        NTT(lr_ntt_host_limb(q, 0, 0, h.data(), h.data()));
        NTT(lr_ntt_host_limb(q, NQ - 1, 1, h.data(), h.data() + C.N));
    }
    for (lr_poly *x : {a, b, wide}) OK(lr_poly_free(x));
}

static void rescales(Config &C, int batch) {
    lr_context *q = C.q;
    typedef int (*Div)(lr_context *, lr_poly *);
    for (Div div : {lr_div_floor_by_last_modulus_ntt, lr_div_round_by_last_modulus_ntt, lr_div_floor_by_last_modulus, lr_div_round_by_last_modulus}) {
        lr_poly *r = poly(q, NQ, batch);
        for (int limbs = NQ; limbs >= 2; --limbs) RUN(div(q, r));       // every level
        OK(lr_poly_set_limbs(r, 3));
        RUN(div(q, r));                                                  // ... and once more on warm tables
        OK(lr_poly_free(r));
    }
    typedef int (*Many)(lr_context *, lr_poly *, int, int);
    for (Many many : {lr_div_floor_by_last_modulus_many, lr_div_round_by_last_modulus_many})
        for (int ntt_domain = 0; ntt_domain < 2; ++ntt_domain) {
            lr_poly *r = poly(q, NQ, batch);
            RUN(many(q, r, 2, ntt_domain));
            RUN(many(q, r, 1, ntt_domain));
            if (ntt_domain) RUN(many(q, r, 0, ntt_domain));              // the two transforms alone
            OK(lr_poly_free(r));
        }
    for (int limbs : {NQ, 3, 2}) {
        lr_poly *r0 = poly(q, limbs, batch), *r1 = poly(q, limbs, batch), *both = poly(q, limbs, 2 * batch);
        RUN(lr_ckks_rescale(C.pl, r0, r1));
        OK(lr_poly_set_limbs(r0, limbs));
        OK(lr_poly_set_limbs(r1, limbs));
        RUN(lr_ckks_rescale(C.pl, r1, r0));
        void *base = nullptr;
        OK(lr_poly_info(both, nullptr, nullptr, nullptr, &base));
        lr_poly *lo = nullptr, *hi = nullptr;                            // two batches laid out back to back
        OK(lr_poly_wrap(q, base, limbs, batch, &lo));
        OK(lr_poly_wrap(q, (uint64_t *)base + (size_t)batch * limbs * C.N, limbs, batch, &hi));
        RUN(lr_ckks_rescale(C.pl, lo, hi));
        for (lr_poly *x : {r0, r1, both, lo, hi}) OK(lr_poly_free(x));
    }
}

static void moddowns(Config &C, int batch) {
    lr_context *q = C.q;
    lr_poly *qp = poly(q, NQ + NP, batch), *pq = poly(q, NQ, batch), *pp = poly(C.p, NP, batch), *out = poly(q, NQ, batch);
    for (int level : {0, 1, NQ - 1}) {
        RUN(lr_moddown_ntt_pq(C.bx, level, qp, out));
        RUN(lr_moddown_split_ntt_pq(C.bx, level, pq, pp, out));
        RUN(lr_moddown_split_ntt_pq(C.bx, level, pq, pp, pq));          // over its own Q part
    }
    for (lr_poly *x : {qp, pq, pp, out}) OK(lr_poly_free(x));
}

static void galois(Config &C, int batch) {
    lr_context *q = C.q;
    lr_poly *a = poly(q, NQ, batch), *b = poly(q, NQ, batch), *wide = poly(q, NQ + 1, batch);
    for (uint64_t deg : {(uint64_t)0, (uint64_t)3, C.N, 2 * C.N + 1}) {
        RUN(lr_mult_by_monomial(q, a, deg, b));
        RUN(lr_mult_by_monomial(q, a, deg, a));
        RUN(lr_mult_by_monomial(q, wide, deg, a));
    }
    for (uint64_t n : {(uint64_t)0, (uint64_t)1, C.N - 1, C.N}) {   // (copies only: no kernel)
        OK(lr_shift(q, a, n, b));
        OK(lr_shift(q, a, n, a));
        OK(lr_shift(q, a, n, wide));
    }
    for (uint64_t gen : {(uint64_t)5, 2 * C.N - 1, 4 * C.N + 25}) {
        RUN(lr_permute(q, a, gen, b));
        RUN(lr_permute(q, wide, gen, b));
        for (int level : {0, NQ - 1}) RUN(lr_permute_ntt(q, level, a, gen, wide));
    }
    for (lr_poly *x : {a, b, wide}) OK(lr_poly_free(x));
}

static void key_switch(Config &C, int batch) {
    lr_context *q = C.q;
    const int beta = (NQ + NP - 1) / NP;
    lr_poly *key = poly(q, NQ + NP, 2 * beta), *a = poly(q, NQ, batch), *o0 = poly(q, NQ, batch), *o1 = poly(q, NQ, batch);
    for (int level : {1, NQ - 1}) RUN(lr_ckks_switch_keys(C.pl, level, a, key, o0, o1));
    for (lr_poly *x : {key, a, o0, o1}) OK(lr_poly_free(x));
}

static void refusals(Config &C) {
    lr_context *q = C.q;
    lr_poly *a = poly(q, NQ, 2), *b = poly(q, NQ, 2), *three = poly(q, NQ, 3), *narrow = poly(q, 2, 2), *one = poly(q, 1, 2), *wide = poly(q, NQ + 1, 2);
    std::vector<uint64_t> h((size_t)NQ * C.N, 1);
    const uint64_t *in[NQ];
    uint64_t *out[NQ];
    for (int i = 0; i < NQ; ++i) in[i] = out[i] = h.data() + (size_t)i * C.N;

    for (auto f : {lr_ntt, lr_intt}) {
        REFUSED(f(nullptr, 0, a, b), LR_ERR_ARG);
        REFUSED(f(q, 0, nullptr, b), LR_ERR_ARG);
        REFUSED(f(q, 0, a, nullptr), LR_ERR_ARG);
        REFUSED(f(q, -1, a, b), LR_ERR_SHAPE);
        REFUSED(f(q, NQ, a, b), LR_ERR_SHAPE);
        REFUSED(f(q, NQ, wide, wide), LR_ERR_SHAPE);
        REFUSED(f(q, 2, a, narrow), LR_ERR_SHAPE);
        REFUSED(f(q, 2, narrow, b), LR_ERR_SHAPE);
        REFUSED(f(q, 1, a, three), LR_ERR_SHAPE);
    }
    for (auto f : {lr_ntt_limb, lr_intt_limb}) {
        REFUSED(f(nullptr, 0, a, 0, b, 0), LR_ERR_ARG);
        REFUSED(f(q, 0, a, 0, nullptr, 0), LR_ERR_ARG);
        REFUSED(f(q, -1, a, 0, b, 0), LR_ERR_SHAPE);
        REFUSED(f(q, NQ, a, 0, b, 0), LR_ERR_SHAPE);
        REFUSED(f(q, 0, a, NQ, b, 0), LR_ERR_SHAPE);
        REFUSED(f(q, 0, a, 0, b, -1), LR_ERR_SHAPE);
        REFUSED(f(q, 0, a, 0, narrow, 2), LR_ERR_SHAPE);
        REFUSED(f(q, 0, a, 0, three, 0), LR_ERR_SHAPE);
    }
    for (auto f : {lr_ntt_host, lr_intt_host}) {
        REFUSED(f(nullptr, 0, in, out), LR_ERR_ARG);
        REFUSED(f(q, 0, nullptr, out), LR_ERR_ARG);
        REFUSED(f(q, 0, in, nullptr), LR_ERR_ARG);
        REFUSED(f(q, -1, in, out), LR_ERR_SHAPE);
        REFUSED(f(q, NQ, in, out), LR_ERR_SHAPE);
    }
    REFUSED(lr_ntt_host_limb(nullptr, 0, 0, h.data(), h.data()), LR_ERR_ARG);
    REFUSED(lr_ntt_host_limb(q, 0, 0, nullptr, h.data()), LR_ERR_ARG);
    REFUSED(lr_ntt_host_limb(q, NQ, 1, h.data(), h.data()), LR_ERR_SHAPE);
    REFUSED(lr_ntt_host_limb(q, -1, 0, h.data(), h.data()), LR_ERR_SHAPE);

    for (auto f : {lr_div_floor_by_last_modulus_ntt, lr_div_round_by_last_modulus_ntt, lr_div_floor_by_last_modulus, lr_div_round_by_last_modulus}) {
        REFUSED(f(nullptr, a), LR_ERR_ARG);
        REFUSED(f(q, nullptr), LR_ERR_ARG);
        REFUSED(f(q, one), LR_ERR_SHAPE);
        REFUSED(f(q, wide), LR_ERR_SHAPE);
    }
    for (auto f : {lr_div_floor_by_last_modulus_many, lr_div_round_by_last_modulus_many})
        for (int ntt_domain = 0; ntt_domain < 2; ++ntt_domain) {
            REFUSED(f(nullptr, a, 1, ntt_domain), LR_ERR_ARG);
            REFUSED(f(q, one, 0, ntt_domain), LR_ERR_SHAPE);
            REFUSED(f(q, a, -1, ntt_domain), LR_ERR_SHAPE);
            REFUSED(f(q, a, NQ, ntt_domain), LR_ERR_SHAPE);
        }
    REFUSED(lr_ckks_rescale(nullptr, a, b), LR_ERR_ARG);
    REFUSED(lr_ckks_rescale(C.pl, a, nullptr), LR_ERR_ARG);
    REFUSED(lr_ckks_rescale(C.pl, one, one), LR_ERR_SHAPE);
    REFUSED(lr_moddown_ntt_pq(nullptr, 0, wide, a), LR_ERR_ARG);
    REFUSED(lr_moddown_ntt_pq(C.bx, 0, nullptr, a), LR_ERR_ARG);
    REFUSED(lr_moddown_ntt_pq(C.bx, NQ, wide, a), LR_ERR_SHAPE);
    REFUSED(lr_moddown_split_ntt_pq(C.bx, 0, a, nullptr, b), LR_ERR_ARG);

    REFUSED(lr_mult_by_monomial(nullptr, a, 1, b), LR_ERR_ARG);
    REFUSED(lr_mult_by_monomial(q, a, 1, nullptr), LR_ERR_ARG);
    REFUSED(lr_mult_by_monomial(q, a, 1, three), LR_ERR_SHAPE);
    REFUSED(lr_mult_by_monomial(q, a, 1, narrow), LR_ERR_SHAPE);
    REFUSED(lr_shift(nullptr, a, 1, b), LR_ERR_ARG);
    REFUSED(lr_shift(q, nullptr, 1, b), LR_ERR_ARG);
    REFUSED(lr_shift(q, a, 1, three), LR_ERR_SHAPE);
    REFUSED(lr_shift(q, a, C.N + 1, b), LR_ERR_ARG);
    REFUSED(lr_shift(q, a, ~(uint64_t)0, a), LR_ERR_ARG);
    REFUSED(lr_permute(nullptr, a, 5, b), LR_ERR_ARG);
    REFUSED(lr_permute(q, a, 5, a), LR_ERR_ARG);                     // not in place
    REFUSED(lr_permute(q, a, 5, three), LR_ERR_SHAPE);
    REFUSED(lr_permute(q, narrow, 5, b), LR_ERR_SHAPE);
    REFUSED(lr_permute_ntt(q, 0, nullptr, 5, b), LR_ERR_ARG);
    REFUSED(lr_permute_ntt(q, 0, a, 5, a), LR_ERR_ARG);
    REFUSED(lr_permute_ntt(q, NQ, a, 5, b), LR_ERR_SHAPE);
    REFUSED(lr_permute_ntt(q, 2, a, 5, narrow), LR_ERR_SHAPE);
    for (lr_poly *x : {a, b, three, narrow, one, wide}) OK(lr_poly_free(x));
}

// 65536 polys of one limb at N = 2^16: run_ntt cuts the launch into chunks of 65535 / count polys.  32 GiB of address space, of which the stubs
// touch two pages per row
static void chunked(Config &C) {
    const int batch = 65536;
    const size_t bytes = (size_t)batch * C.N * sizeof(uint64_t);
    void *mem = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    CHECK(mem != MAP_FAILED);
    if (mem == MAP_FAILED) return;
    (void)madvise(mem, bytes, MADV_NOHUGEPAGE);
    lr_context *q = C.q;
    lr_poly *big = nullptr;
    OK(lr_poly_wrap(q, mem, 1, batch, &big));
    unsigned long long before = lr::g_stub_launches.load();
    NTT(lr_ntt(q, 0, big, big));
    CHECK(lr::g_stub_launches.load() - before == 4);                 // two chunks: top pass + sub-blocks each
    before = lr::g_stub_launches.load();
    NTT(lr_intt(q, 0, big, big));
    CHECK(lr::g_stub_launches.load() - before == 2);                 // two chunks on the pair-flag kernels
    NTT(lr_ntt_limb(q, 3, big, 0, big, 0));
    OK(lr_poly_free(big));
    CHECK(munmap(mem, bytes) == 0);
}

// one (ring, moduli, options) configuration: every entry point, then the line of its kernel names
static void run_config(int logn, const Moduli &m, int v) {
    lr_options opt;
    OK(lr_options_init(&opt));
    const char *name = set_option(&opt, v, logn);
    if (!name) return;
    Config C;
    C.N = (uint64_t)1 << logn;
    OK(lr_context_create_ex(C.N, m.q, NQ, 0, &opt, &C.q));
    OK(lr_context_create_ex(C.N, P, NP, 0, &opt, &C.p));
    OK(lr_bext_create(C.q, C.p, &C.bx));
    OK(lr_ckks_plan_create_ex(C.q, C.p, 2 * MAXB, &opt, &C.pl));
    int fwd = -2, inv = -2;
    OK(lr_context_ntt_variants(C.q, &fwd, &inv));
    if (v == 0 && m.fwd != -2) CHECK(fwd == m.fwd);
    if (v == 1) CHECK(fwd == -1 && inv == -1);
    const int fail_before = g_fail;
    for (int batch : {1, MAXB}) {
        transforms(C, batch);
        rescales(C, batch);
        moddowns(C, batch);
        galois(C, batch);
        key_switch(C, batch);
    }
    refusals(C);
    if (logn == 16 && v == 0 && &m == &kModuli[0]) chunked(C);
    if (g_fail != fail_before) std::fprintf(stderr, "... at N = 2^%d, moduli %s, %s\n", logn, m.name, name);
    std::printf("routes N=2^%d moduli=%s %s fwd=%d inv=%d:", logn, m.name, name, fwd, inv);
    for (const std::string &s : C.names) std::printf(" %s", s.c_str());
    std::printf("\n");
    OK(lr_ckks_plan_destroy(C.pl));
    OK(lr_bext_destroy(C.bx));
    OK(lr_context_destroy(C.q));
    OK(lr_context_destroy(C.p));
}

int main(int argc, char **argv) {
    for (int logn : kLogN)
        for (const Moduli &m : kModuli)
            for (int v = 0; v < 13; ++v) run_config(logn, m, v);
    // the classes of the command line: "name q0 .. q4" each, fwd = -2 (no expectation here: the test compares the printed variants with its own
    // restatement of the admission predicates)
    for (int a = 1; a + NQ < argc; a += NQ + 1) {
        Moduli m{argv[a], {}, -2};
        for (int i = 0; i < NQ; ++i) m.q[i] = std::strtoull(argv[a + 1 + i], nullptr, 10);
        for (int logn : kLogN)
            for (int v : {0, 1, 13, 8, 9}) run_config(logn, m, v);
    }
    return driver_end(ALLOCATIONS, g_refusals, "ntt_dispatch: calls %d, refusals %d", g_calls.load(), g_refusals.load());
}
