// lr_ckks_chain.cpp -- C ABI: lr_ckks_rotate_chain, a chain of evaluator.permuteNTT steps (ckks/evaluator.go:1452-1471) on an
// lr_ckks_plan as one call.  Over a state (a0, a1) on Q[0..level], NTT domain, step i with Galois element g_i and key K_i is
//   (e0, e1) = (PermuteNTT(a0, g_i), PermuteNTT(a1, g_i))     (p0, p1) = switchKeysInPlace(level, e1, K_i)     (r0, r1) = (CRed(e0 + p0), p1)
//   replace:     (a0, a1) <- (r0, r1)                               rotateColumnsPow2, :1414-1423
//   accumulate:  (a0, a1) <- (CRed(r0 + a0), CRed(r1 + a1))         RotateColumns(ct, ., tmp); Add(ct, tmp, ct): the slot-sum loop
// The fused route of an accumulating chain makes ONE pass in front of the key switch (launch_ckks_chain_step, lr_ckks_chain.hip: the key
// switch's input and the first component's addend, the running sum already in it) and hands the running second component to the key
// switch's last pass as its other addend: no Add is left.  The composed route is lr_ckks_rotate's body per step and two LR_ADD when
// accumulating; a replacing chain, which has no Add to lose, always takes it (chain_route).  Same bits on both for a state in [0, q).
// The unit's name keeps it out of the lr_abi_*.cpp set that the shared sanitizer build links against its fixed launch stubs: the launcher
// it calls has a stand-in of its own (tests/cpp/ckks_chain_stub.cpp).
#include "lr_host.hpp"

namespace lr_host {
namespace {

const char *const kWho = "ckks rotate chain: ";
int refuse(int code, const char *what) { return fail(code, std::string(kWho) + what); }

// a component of a ciphertext: the caller's poly or one half of a pool pair
struct Comp {
    u64 *d;
    long long stride;
    Comp(u64 *d_, long long stride_) : d(d_), stride(stride_) {}
    Comp(const lr_poly *p) : d(p->d), stride(p->stride()) {}
};

enum class ChainRoute { Fused, Composed };
// THE route decision of a CKKS chain.  An accumulating chain takes the fused step wherever the key switch's last pass
// takes addends inside the forward transform (ntt_epilogue_ok), unless the plan or its context asks for the call-by-call shape
// (lr_options::no_epilogue); a batch beyond the step pass's grid goes call by call as well.  A REPLACING chain is composed everywhere, as
// measured (one MI355X, DESIGN.md 6.2, the fused step against the RotateColumnsPow2 host loop in the same run, medians of 5): the pass in
// front of the key switch only stands for the two gathers that lr_ckks_rotate launches anyway, and no regime beat the host loop by more
// than the spread of the repeated medians -- PN15QP880 top level, one ciphertext 2272.9 us against 2276.8 (spread 18 and 33), 256
// ciphertexts 159.87 ms against 159.32 (0.68 and 0.79); PN16QP1761 top level, one ciphertext 7852.5 us against 7871.5 (32 and 34), 64
// ciphertexts 225.89 ms against 224.06 (1.10 and 1.72).  The slot sum is where the Add disappears: 2284.0 us against 2407.0 and 163.64 ms
// against 177.37 at PN15QP880, 7777.2 us against 8136.2 and 230.95 ms per 64 against 245.27 at PN16QP1761.
ChainRoute chain_route(const lr_ckks_plan *pl, int batch, bool accumulate) {
    if (!accumulate) return ChainRoute::Composed;
    if (pl->opt.no_epilogue || pl->cQ->opt.no_epilogue) return ChainRoute::Composed;
    if (!ntt_epilogue_ok(pl->cQ)) return ChainRoute::Composed;
    if (batch > 32767) return ChainRoute::Composed;
    return ChainRoute::Fused;
}

// the chain itself; every argument checked
int chain_core(lr_ckks_plan *pl, int level, const lr_poly *c0, const lr_poly *c1, int n_steps, const u64 *gens, const lr_poly *const *keys,
               bool accumulate, lr_poly *o0, lr_poly *o1) {
    lr_context *cQ = pl->cQ;
    const int batch = c0->batch, L1 = level + 1, n = (int)cQ->h.N;
    const long long s = (long long)L1 * n;
    LR_TRY(begin_pipeline(pl));
    const bool fused = chain_route(pl, batch, accumulate) == ChainRoute::Fused;
    Comp a[2] = {c0, c1};
    const Comp out[2] = {o0, o1};
    // A replacing step's inputs are dead once they are permuted (both gathers come before the key switch writes anything): every step
    // writes the caller's outputs, in place from the second step on, whichever polys they are.  An accumulating step reads its state
    // again while it writes -- the fused route in the key switch's last pass, the composed one in its two Adds -- so there an output
    // over the OTHER component's input needs the state to start as a copy, and the fused route keeps the state off its destination.
    const bool crossed = out[0].d == a[1].d || out[1].d == a[0].d;
    const bool pools = accumulate || (crossed && n_steps == 0);
    if (pools)
        for (Pool *p : {&pl->bfvP, &pl->chainP}) LR_TRY(p->ensure(cQ, (size_t)2 * batch * s));
    for (Pool *p : {&pl->c0, &pl->c2x, &pl->q1, &pl->q2}) LR_TRY(p->ensure(cQ, (size_t)batch * s));
    u64 *const pair[2] = {pl->bfvP.d, pl->chainP.d};       // each [2][batch][level + 1][N]
    const KeySwitchAcc acc{{pl->q1.d, pl->q2.d}, {s, s}};
    auto copy = [&](const Comp &in, const Comp &dst) -> int {
        return in.d == dst.d ? (int)LR_OK : run_ewise(cQ, LR_COPY, L1, batch, in.d, in.stride, nullptr, 0, dst.d, dst.stride, nullptr);
    };
    int next = 0;      // the pool pair the next accumulating step writes; the state is never there
    if (pools && crossed) {
        for (int k = 0; k < 2; ++k) {
            const Comp dst(pair[1] + (long long)k * batch * s, s);
            LR_TRY(copy(a[k], dst));
            a[k] = dst;
        }
    }
    if (n_steps == 0) {
        for (int k = 0; k < 2; ++k) LR_TRY(copy(a[k], out[k]));
        return LR_OK;
    }
    for (int i = 0; i < n_steps; ++i) {
        const bool last = i == n_steps - 1;
        const Comp p[2] = {Comp(pair[next], s), Comp(pair[next] + (long long)batch * s, s)};
        if (fused) {
            // (accumulating: chain_route sends no replacing chain here)
            const Comp dst[2] = {last ? out[0] : p[0], last ? out[1] : p[1]};
            CkksChainStepLaunch S;
            S.a0 = a[0].d; S.a0_stride = a[0].stride; S.a1 = a[1].d; S.a1_stride = a[1].stride;
            S.plus0 = pl->c0.d; S.cx = pl->c2x.d; S.plus_stride = S.cx_stride = s;
            S.n = n; S.logn = (int)cQ->h.logN;
            S.gen = (u32)(gens[i] & ((cQ->h.N << 1) - 1));
            S.lp = cQ->d_lp;
            LR_HIP(launch_ckks_chain_step(S, L1, batch, cQ->stream));                                                 // :1458-1459 and Add, first component
            // The running second component is the last pass's other addend.  Where that pass would write the poly it adds -- a one-step
            // chain in place -- the result goes through the pool and is copied once: the transform epilogue and submul_kernel both load
            // the addend of an element before the same lane stores it, but nothing of the chain should hang on every variant of the
            // transform kernels keeping that order, for the sake of one copy in a chain of one step.
            const Comp w1 = dst[1].d == a[1].d ? p[1] : dst[1];
            KeySwitchEpilogue fin{dst[0].d, w1.d, dst[0].stride, pl->c0.d, a[1].d, s};
            fin.out1_stride = w1.stride;
            fin.plus1_stride = a[1].stride;
            LR_TRY(switch_keys_core(pl, level, batch, pl->c2x.d, s, keys[i], acc, &fin));                             // :1464-1467 and Add, second component
            LR_TRY(copy(w1, dst[1]));
            a[0] = dst[0];
            a[1] = dst[1];
            next ^= 1;
            continue;
        }
        // lr_ckks_rotate's body; an accumulating step rotates into a pool pair and adds the state to it
        const Comp r[2] = {accumulate ? p[0] : out[0], accumulate ? p[1] : out[1]};
        const ComponentPair ins = component_pair(a[0].d, a[0].stride, a[1].d, a[1].stride, batch);
        if (batch == 1 && !pl->opt.no_pair && ins) {
            // one ciphertext: both components in one launch, the strides are the distances between them
            LR_TRY(run_permute_ntt(cQ, L1, 2, a[0].d, ins.stride, pl->c0.d, component_distance(pl->c0.d, pl->c2x.d), gens[i]));     // :1458-1459
        } else {
            LR_TRY(run_permute_ntt(cQ, L1, batch, a[0].d, a[0].stride, pl->c0.d, s, gens[i]));                        // :1458
            LR_TRY(run_permute_ntt(cQ, L1, batch, a[1].d, a[1].stride, pl->c2x.d, s, gens[i]));                       // :1459
        }
        KeySwitchEpilogue fin{r[0].d, r[1].d, r[0].stride, pl->c0.d, nullptr, s};
        fin.out1_stride = r[1].stride;
        LR_TRY(switch_keys_core(pl, level, batch, pl->c2x.d, s, keys[i], acc, &fin));                                 // :1464-1467
        if (accumulate)
            for (int k = 0; k < 2; ++k)
                LR_TRY(run_ewise(cQ, LR_ADD, L1, batch, a[k].d, a[k].stride, r[k].d, r[k].stride, out[k].d, out[k].stride, nullptr));     // Add(ct, tmp, ct)
        a[0] = out[0];
        a[1] = out[1];
    }
    return LR_OK;
}

}  // namespace
}  // namespace lr_host

extern "C" int lr_ckks_rotate_chain(lr_ckks_plan *pl, int level, const lr_poly *c0, const lr_poly *c1, int n_steps, const uint64_t *gens,
                                    const lr_poly *const *keys, int accumulate, lr_poly *o0, lr_poly *o1) {
    return guarded([&]() -> int {
    // LR_ERR_ARG
    if (!pl || !c0 || !c1 || !o0 || !o1) return refuse(LR_ERR_ARG, "null argument");
    if (n_steps < 0) return refuse(LR_ERR_ARG, "negative step count");
    if (n_steps > 0 && (!gens || !keys)) return refuse(LR_ERR_ARG, "null argument");
    for (int i = 0; i < n_steps; ++i) {
        if (!keys[i]) return refuse(LR_ERR_ARG, "null argument");
        if (!(gens[i] & 1)) return refuse(LR_ERR_ARG, "a Galois element must be odd");
    }
    if (o0 == o1 || o0->d == o1->d) return refuse(LR_ERR_ARG, "the two output polys must be distinct");
    // LR_ERR_SHAPE
    LR_TRY(check_call(pl, level, c0->batch, {c0, c1, o0, o1}));
    const int alpha = pl->dec->alpha, beta = (level + 1 + alpha - 1) / alpha;
    for (int i = 0; i < n_steps; ++i)
        if (keys[i]->N != pl->cQ->h.N || keys[i]->batch < 2 * beta || keys[i]->limbs < pl->cQ->h.L() + pl->cP->h.L())
            return refuse(LR_ERR_SHAPE, "rotation key: need batch >= 2*beta and |Q|+|P| limbs");
    if (pl->cQ->h.N < 2 || pl->cQ->h.logN > 30) return refuse(LR_ERR_UNSUPPORTED, "ring degree");
    return chain_core(pl, level, c0, c1, n_steps, gens, keys, accumulate != 0, o0, o1);
    });
}
