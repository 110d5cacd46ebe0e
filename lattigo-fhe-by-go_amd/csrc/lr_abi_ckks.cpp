// lr_abi_ckks.cpp -- C ABI: lr_ckks_plan, the key switch itself (ks_*, switch_keys_core, bfv_switch_keys_core / _grouped), the checks the
// pipelines' entry points share, and the calls that sit on the key switch's own stages or beside it: switchKeysInPlace, the hoisted
// rotations (they take the decomposition and the inner product apart), pk-encrypt and decrypt.  The evaluators' pipelines over the key
// switch are lr_abi_ckks_eval.cpp (MulRelin, rotations and chains, Rescale, the power basis) and lr_abi_bfv_eval.cpp.
#include "lr_host.hpp"

namespace lr_host {
// live plans per device that are not lanes of a batcher: one = a lone evaluator, whose small launches may run side by side (PlanFork)
std::atomic<int> &standalone_plans(int device) {
    static std::atomic<int> counts[64];
    return counts[device >= 0 && device < 64 ? device : 0];
}
}  // namespace lr_host

extern "C" int lr_ckks_plan_create(lr_context *cQ, lr_context *cP, int max_batch, lr_ckks_plan **out) {
    return lr_ckks_plan_create_ex(cQ, cP, max_batch, nullptr, out);
}

extern "C" int lr_ckks_plan_create_ex(lr_context *cQ, lr_context *cP, int max_batch, const lr_options *options, lr_ckks_plan **out) {
    return guarded([&]() -> int {
    if (!cQ || !cP || !out) return fail(LR_ERR_ARG, "null argument");
    *out = nullptr;
    Options parsed = cQ->opt;                                   // options == NULL: the options of ctxQ, as the header says
    if (options) LR_TRY(options_from_public(options, &parsed));
    else parsed.apply_env();
    if (max_batch < 1) return fail(LR_ERR_ARG, "max_batch must be >= 1");
    LR_TRY(same_degree(cQ, cP));
    std::unique_ptr<lr_ckks_plan> p(new lr_ckks_plan());
    p->cQ = cQ;
    p->cP = cP;
    p->device = cQ->device;
    p->max_batch = max_batch;
    p->opt = parsed;
    LR_TRY(lr_bext_create(cQ, cP, &p->bext));
    int rc = lr_decomposer_create(cQ, cP, &p->dec);
    if (rc != LR_OK) {
        lr_bext_destroy(p->bext);
        return rc;
    }
    standalone_plans(p->device).fetch_add(1);
    *out = p.release();
    return LR_OK;
    });
}

extern "C" int lr_ckks_plan_stats(const lr_ckks_plan *p, uint64_t *forks, uint64_t *grouped_extensions) {
    return guarded([&]() -> int {
    if (!p) return fail(LR_ERR_ARG, "null plan");
    if (forks) *forks = p->forks;
    if (grouped_extensions) *grouped_extensions = p->grouped_ext;
    return LR_OK;
    });
}

extern "C" int lr_ckks_plan_destroy(lr_ckks_plan *p) {
    return guarded([&]() -> int {
    if (!p) return LR_OK;
    if (p->lane_of) return fail(LR_ERR_ARG, "this plan is a lane of a live batcher: destroy the batcher first (it holds the plan and its contexts)");
    (void)hipSetDevice(p->device);
    (void)hipDeviceSynchronize();   // the handle's work may be on its contexts' caller-supplied stream
    lr_bext_destroy(p->bext);
    lr_decomposer_destroy(p->dec);
    if (p->ev_fork) (void)hipEventDestroy(p->ev_fork);
    if (p->ev_join) (void)hipEventDestroy(p->ev_join);
    if (p->aux) (void)hipStreamDestroy(p->aux);
    standalone_plans(p->device).fetch_sub(1);
    delete p;
    return LR_OK;
    });
}

namespace lr_host {

// Two independent launches of one pipeline side by side: between the constructor and join() the calling thread's forward transforms go
// to the plan's auxiliary stream, which starts behind everything enqueued on the contexts' stream so far; join() makes the contexts'
// stream wait for them.  Worth it only on an otherwise idle device and while the forked launch is far from filling it
// (Options::fork_below_workgroups, 256).  "Otherwise idle" is a structural test, not a momentary one: the plan is the only one alive on its device that is not a
// batcher's lane -- the lone evaluator, for whom latency is what there is.
// Tried and dropped (profiles/r03/fork_policies.txt): forking whenever the launch is small (sixteen threads with a plan each lose a
// quarter of their rate), counting the calls being enqueued at the moment (the count is below the threads most of the time), auxiliary
// streams shared between plans (unrelated pipelines queue behind each other's fork events), an auxiliary stream created with every
// plan (twice the streams on the runtime's four hardware queues: slower without a single fork), lanes of a batcher that fork while
// they are the only lane running (13.4 k products/s against 12.5 k from a C++ host at sixteen callers, 10.5 k against 13.6 k from
// Python threads: the extra streams share hardware queues with the lanes' own, see GPU_MAX_HW_QUEUES in DESIGN 9).
// Capturable: the auxiliary stream joins the capture at the fork and leaves it at the join (it is created by the first fork, i.e. in
// the warm-up call the capture contract asks for).
struct PlanFork {
    lr_ckks_plan *pl;
    bool on = false;
    int rc = LR_OK;
    PlanFork(lr_ckks_plan *p, int workgroups) : pl(p) {
        if (pl->opt.no_fork || pl->fork_failed || g_fork_stream) return;
        // ... and only where one workgroup of the forked launch runs long enough to pay for the two stream hand-overs (~ 19 us): the
        // 2^15 sub-blocks of N = 2^16 (42 us).  Since small 2^15 launches run on 2^14 sub-blocks (20 us, like the 2^14 kernels) a fork
        // there costs more than it hides: PN15QP880 batch 1 4.64 k products/s forked, 5.06 k in order; PN14QP438 6.42 k / 7.30 k;
        // PN16QP1761 1.69 k / 1.64 k (profiles/r03/fork_policies.txt).
        if (pl->cQ->h.logN != 16) return;
        if (pl->lane_of || standalone_plans(pl->device).load(std::memory_order_relaxed) != 1 || workgroups >= pl->opt.fork_below_workgroups) return;
        if (!pl->aux) {
            if (create_stream(&pl->aux, 1) != hipSuccess ||
                hipEventCreateWithFlags(&pl->ev_fork, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&pl->ev_join, hipEventDisableTiming) != hipSuccess) {
                (void)hipGetLastError();
                pl->fork_failed = true;   // the pipelines stay in order on one stream
                return;
            }
        }
        hipError_t e = hipEventRecord(pl->ev_fork, pl->cQ->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(pl->aux, pl->ev_fork, 0);
        if (e != hipSuccess) {
            rc = fail(LR_ERR_HIP, std::string("fork: ") + hipGetErrorString(e));
            return;
        }
        on = true;
        pl->forks += 1;
        g_fork_stream = pl->aux;
    }
    // the launches that follow go to the contexts' stream again (and run beside the forked ones until join())
    void back() {
        if (on) g_fork_stream = nullptr;
    }
    int join() {
        if (!on) return LR_OK;
        on = false;
        g_fork_stream = nullptr;
        hipError_t e = hipEventRecord(pl->ev_join, pl->aux);
        if (e == hipSuccess) e = hipStreamWaitEvent(pl->cQ->stream, pl->ev_join, 0);
        if (e != hipSuccess) return fail(LR_ERR_HIP, std::string("join: ") + hipGetErrorString(e));
        return LR_OK;
    }
    ~PlanFork() { (void)join(); }   // error paths: the contexts' stream still waits for whatever was forked
};


// Context.Permute (coefficient domain) or PermuteNTT of `batch` polys: THE GaloisLaunch fill of the rotations, CKKS and BFV
int run_permute(lr_context *c, bool ntt_domain, int limbs, int batch, const u64 *in, long long in_stride, u64 *out, long long out_stride,
                u64 gen, const u64 *const *in_table) {
    GaloisLaunch L;
    L.in_table = in_table;
    L.in = in;
    L.out = out;
    L.in_stride = in_stride;
    L.out_stride = out_stride;
    L.n = (int)c->h.N;
    L.logn = (int)c->h.logN;
    L.ntt_domain = ntt_domain ? 1 : 0;
    L.gen = gen & ((c->h.N << 1) - 1);
    L.lp = c->d_lp;
    LR_HIP(launch_permute(L, limbs, batch, c->stream));
    return LR_OK;
}
int run_permute_ntt(lr_context *c, int limbs, int batch, const u64 *in, long long in_stride, u64 *out, long long out_stride,
                    u64 gen, const u64 *const *in_table) {
    return run_permute(c, true, limbs, batch, in, in_stride, out, out_stride, gen, in_table);
}

// ------------------------------------------------------------------------------------------
// the key switch: ks_decompose, then ks_inner_product, then one of the two ModDown tails
// ------------------------------------------------------------------------------------------
namespace {

struct KsSizes {
    int beta;                    // digits at this level, :1508
    long long sQ, sP, dQ, dP;    // words of one poly over Q / over P, and of one digit (`batch` polys) over Q / over P
};
KsSizes ks_sizes(const lr_ckks_plan *pl, int level, int batch) {
    const int alpha = pl->dec->alpha;
    const long long n = (long long)pl->cQ->h.N, sQ = pl->cQ->h.L() * n, sP = pl->cP->h.L() * n;
    return {(level + 1 + alpha - 1) / alpha, sQ, sP, batch * sQ, batch * sP};
}

// where the decomposition's input is and where the limbs a digit owns come from
enum class KsInput {
    Ntt,          // ckks: cx in the NTT domain, the digits come from InvNTT(cx); the own limbs are cx itself, which the inner product reads in place
    NttCopyOwn,   // the same with the own limbs copied into the digits (the hoisted path permutes whole digits), :1579-1584
    Coeff,        // bfv.switchKeys, bfv/evaluator.go:736-770: cx in the coefficient domain -- the digits are decomposed from cx itself and the
                  // own limbs are NTT(cx) (:753, kept in pl->c2)
};

// what ks_decompose launches, decided once from the level, the batch and the plan's options
struct KsDecomposition {
    KsSizes z;
    int full;         // leading digits that own exactly alpha limbs at this level: their transforms share one launch
    bool exttop;      // the digits' extensions apply the top stage of the forward transforms that follow them
    bool invtop;      // ... and the last stage and the scaling of the inverse transform in front of them
    bool staged;      // the extensions land in staging buffers and the transforms go out of place
};
KsDecomposition ks_plan_decomposition(const lr_ckks_plan *pl, int level, int batch, bool coeff_input) {
    const lr_context *cQ = pl->cQ, *cP = pl->cP;
    const lr_decomposer *dec = pl->dec;
    const int nP = cP->h.L(), n = (int)cQ->h.N, alpha = dec->alpha;
    KsDecomposition d;
    d.z = ks_sizes(pl, level, batch);
    const int beta = d.z.beta;
    // N = 2^16: a forward transform whose input and output rows are disjoint computes its top stage while loading (one
    // launch); in place it needs a separate streaming pass first.  The extensions therefore land in staging buffers of the
    // same shape and the transforms write the pools the consumers read.
    const bool asm16 = cQ->h.logN == 16 && cQ->use_asm && cQ->asm_fwd >= 0 && cP->use_asm && cP->asm_fwd >= 0;
    // N = 2^15 and a key switch whose largest transform launch is small: the same arrangement on the 2^14 sub-block kernels (the
    // extension applies the stage over bit 14, run_ntt_launch takes pretop as the decision for the split)
    const bool asm15 = cQ->h.logN == 15 && ntt_split15(cQ, (long long)std::max(1, level + 1 - alpha) * beta * batch) &&
                       ntt_split15(cP, (long long)nP * beta * batch);
    // ... or, better, the extension itself applies the stage over index bit 15 (each of its threads holds the coefficients j and
    // j + N/2) and the plain sub-block kernels transform in place, reading their own half only.  Possible when every digit of
    // this level goes through the sum-form extension kernel (no trivial-copy digit).
    d.exttop = (asm16 || asm15) && !pl->opt.no_exttop;
    // the digits' extensions apply the top stage of the transforms that follow them (exttop): then they also take the last stage and
    // the scaling of the inverse transform in front of them (its sub-blocks leave the rows lazy; nothing else reads c2 on this path)
    d.invtop = !coeff_input && !pl->opt.no_invtop && cQ->asm_inv >= 0;
    d.full = 0;
    for (int i = 0; i < beta; ++i) {
        const DigitShape g = digit_shape(dec, level, i);
        if (g.full && d.full == i) ++d.full;
        d.exttop = d.exttop && g.extended && ext_top_supported(g.modup->tables(), g.n_in(), n);
        d.invtop = d.invtop && g.extended && g.modup->invtop0 != nullptr && g.n_in() <= 8;
    }
    d.invtop = d.invtop && d.exttop;
    d.staged = asm16 && !d.exttop && !pl->opt.no_staging;
    return d;
}

// Digit decomposition of switchKeysInPlace / RotateHoisted (ckks/evaluator.go:1503-1510, 1258-1272, 1561-1591) and of bfv.switchKeys:
// pl->c2QiQ = [beta][batch][|Q|][N], pl->c2QiP = [beta][batch][|P|][N], both in the NTT domain, without the limbs a digit owns unless
// KsInput::NttCopyOwn.
int ks_decompose(lr_ckks_plan *pl, int level, int batch, const u64 *cx, long long cx_stride, KsInput input) {
    lr_context *cQ = pl->cQ, *cP = pl->cP;
    lr_decomposer *dec = pl->dec;
    const int nP = cP->h.L(), n = (int)cQ->h.N, alpha = dec->alpha;
    const bool coeff_input = input == KsInput::Coeff;
    const KsDecomposition d = ks_plan_decomposition(pl, level, batch, coeff_input);
    const int beta = d.z.beta;
    const long long sQ = d.z.sQ, sP = d.z.sP, dQ = d.z.dQ, dP = d.z.dP;
    const bool exttop = d.exttop;
    LR_TRY(pl->c2QiQ.ensure(cQ, (size_t)beta * dQ));
    LR_TRY(pl->c2.ensure(cQ, (size_t)batch * sQ));
    LR_TRY(pl->c2QiP.ensure(cQ, (size_t)beta * dP));
    if (d.staged) {
        LR_TRY(pl->stageQ.ensure(cQ, (size_t)beta * dQ));
        LR_TRY(pl->stageP.ensure(cQ, (size_t)beta * dP));
    }
    u64 *const outQ = pl->c2QiQ.d, *const outP = pl->c2QiP.d;
    u64 *const srcQ = d.staged ? pl->stageQ.d : outQ, *const srcP = d.staged ? pl->stageP.d : outP;     // where the extensions land

    // the input transform: ckks :1503 (InvNTT) / bfv :753 (NTT)
    const Rows cxr{const_cast<u64 *>(cx), cx_stride, 0, 1}, c2r{pl->c2.d, sQ, 0, 1};
    LR_TRY(run_ntt(cQ, !coeff_input, cxr, c2r, 0, 1, level + 1, batch, 0, 0, nullptr, false, d.invtop));
    // (bfv: the decomposition reads the caller's coefficient-domain rows; the transformed copy serves the digits' own limbs)
    const Rows coeffs = coeff_input ? cxr : c2r;

    // the digits' extensions: independent, same shape -> one grouped launch (copy-branch digits launch at once)
    std::vector<ExtPending> pending;
    pending.reserve((size_t)beta);
    const DigitExtension how{exttop, true, d.invtop, pl->opt.no_ext_group ? nullptr : &pending};
    for (int i = 0; i < beta; ++i) {
        const Rows digP{srcP + (long long)i * dP, sP, 0, 1};
        LR_TRY(decompose_core(dec, level, i, coeffs, batch, Rows{srcQ + (long long)i * dQ, sQ, 0, 1}, &digP, how));    // decomposeAndSplitNTT, :1561-1591
        if (input == KsInput::NttCopyOwn) {   // :1579-1584
            const DigitShape g = digit_shape(dec, level, i);
            LR_TRY(run_ewise(cQ, LR_COPY, g.d1 - g.d0, batch, cx + (long long)g.d0 * n, cx_stride, nullptr, 0,
                             outQ + (long long)i * dQ + (long long)g.d0 * n, sQ, nullptr, g.d0));
        }
    }
    LR_TRY(flush_ext(cQ, pending, batch, &pl->grouped_ext));

    // the digits' forward transforms, every row but the own ones
    auto outside_own = [&](int i) -> int {   // the rows below and above the own block of digit i (the digits that are not full: their own launches)
        const DigitShape g = digit_shape(dec, level, i);
        u64 *dq = outQ + (long long)i * dQ, *sq = srcQ + (long long)i * dQ;
        LR_TRY(run_ntt(cQ, false, Rows{sq, sQ, 0, 1}, Rows{dq, sQ, 0, 1}, 0, 1, g.d0, batch, 0, 0, nullptr, exttop));
        return run_ntt(cQ, false, Rows{sq, sQ, g.d1, 1}, Rows{dq, sQ, g.d1, 1}, g.d1, 1, level + 1 - g.d1, batch, 0, 0, nullptr, exttop);
    };
    auto p_rows = [&]() -> int {             // :1590, every digit's P rows: one launch
        return run_ntt(cP, false, Rows{srcP, sP, 0, 1}, Rows{outP, sP, 0, 1}, 0, 1, nP, beta * batch, 0, 0, nullptr, exttop);
    };
    auto full_digits = [&]() -> int {        // the rows outside each full digit's own block, all full digits at once (grid z = digit)
        if (d.full == 0 || level + 1 - alpha <= 0) return LR_OK;
        return run_ntt(cQ, false, Rows{srcQ, sQ, 0, 1}, Rows{outQ, sQ, 0, 1}, 0, 1, level + 1 - alpha, d.full * batch, alpha, batch, nullptr, exttop);
    };
    // the digits' P rows beside their Q rows (another kernel variant, so another launch: at a small batch each fills a fraction of the chip)
    PlanFork forkP(pl, nP * beta * batch);
    LR_TRY(forkP.rc);
    if (forkP.on) {
        // beside the full digits' grouped launch: the P rows and the partial digits' Q rows (PN16QP1761, one ciphertext: 70 + 34 us
        // next to 99 us)
        LR_TRY(p_rows());
        for (int i = d.full; i < beta; ++i) LR_TRY(outside_own(i));
        forkP.back();
        LR_TRY(full_digits());
    } else {
        LR_TRY(full_digits());
        for (int i = d.full; i < beta; ++i) LR_TRY(outside_own(i));
        LR_TRY(p_rows());
    }
    return forkP.join();
}

// exact 128-bit sums in the key inner product: beta products below q^2 each must stay below q * 2^64
bool keymac_wide_ok(const lr_ckks_plan *pl, const lr_context *c, int beta) {
    if (pl->opt.keymac_narrow) return false;
    u64 qmax = 0;
    for (u64 q : c->h.q) qmax = q > qmax ? q : qmax;
    return (u128)qmax * (u128)beta < ((u128)1 << 64);
}

// The digits the inner product reads: [beta][batch][|Q| resp. |P|][N].  Either they lack the limbs they own, which are then read from the
// key switch's NTT-domain input (in_place), or they carry them and may be read through a Galois permutation (whole).  The kernel has no
// permuted read of `own`: build a KsDigits with one of the two factories, which never combine the two.
struct KsDigits {
    const u64 *Q, *P;
    const u64 *own;           // nullptr: inside Q
    long long own_stride;
    u64 perm_gen;             // hoisted rotations: the Galois element the digits are read through (KeyMacLaunch::perm_gen); 0 = as they are
    static KsDigits in_place(const lr_ckks_plan *pl, const u64 *own, long long own_stride) { return {pl->c2QiQ.d, pl->c2QiP.d, own, own_stride, 0}; }
    static KsDigits whole(const u64 *Q, const u64 *P, u64 perm_gen = 0) { return {Q, P, nullptr, 0, perm_gen}; }
};

// the P part of the inner product from its Q part: the digits' P rows and the key's limbs |Q|.. into the two halves of poolPP
KeyMacLaunch keymac_p_part(const lr_ckks_plan *pl, KeyMacLaunch K, const KsSizes &z, const u64 *digP, u64 *pool2P, u64 *pool3P) {
    K.c2 = digP; K.c2_digit_stride = z.dP; K.c2_poly_stride = z.sP;
    K.key_limb0 = pl->cQ->h.L();
    K.out0 = pool2P; K.out1 = pool3P; K.out_stride = K.out1_stride = z.sP;
    K.lp = pl->cP->d_lp;
    K.wide = keymac_wide_ok(pl, pl->cP, z.beta) ? 1 : 0;
    K.own = nullptr; K.own_stride = 0; K.alpha = 0;
    return K;
}

// The members of a pass that one inner product works on: polys [first, first + count) of its `batch`, under a key of their own (the
// grouped BFV key switch, bfv_switch_keys_grouped).  The range is base offsets into the digits, `own`, the accumulators and poolPP; the
// strides stay those of the whole pass.  The default is every member: the launch of a pass under one key.
struct KsMembers {
    int first = 0, count = -1;      // count < 0: all `batch` members
};

// Inner product of the digits with a switching key (:1511-1535 / :1339-1365): acc <- the Q parts, pl->poolPP = [2][batch][|P|][N] <- the
// P parts of sum over the digits of evakey[i][0/1] (*) c2_i, canonical; for the members `mem` of the pass
int ks_inner_product(lr_ckks_plan *pl, int level, int batch, const KsDigits &dig, const lr_poly *evk, const KeySwitchAcc &acc, KsMembers mem = KsMembers()) {
    lr_context *cQ = pl->cQ;
    const int nQ = cQ->h.L(), nP = pl->cP->h.L();
    const KsSizes z = ks_sizes(pl, level, batch);
    const long long m0 = mem.first;
    const int members = mem.count < 0 ? batch : mem.count;
    if (evk->batch < 2 * z.beta || evk->limbs < nQ + nP) return fail(LR_ERR_SHAPE, "evaluation key: need batch >= 2*beta and |Q|+|P| limbs");
    LR_TRY(pl->poolPP.ensure(cQ, (size_t)2 * batch * z.sP));
    KeyMacLaunch KQ;
    KQ.tile8 = 0;
    KQ.perm_gen = (unsigned)(dig.perm_gen & ((cQ->h.N << 1) - 1));
    KQ.n = (int)cQ->h.N; KQ.logn = (int)cQ->h.logN; KQ.beta = z.beta;
    KQ.key = evk->d; KQ.key_poly_stride = evk->stride(); KQ.key_limb0 = 0;
    KQ.c2 = dig.Q + m0 * z.sQ; KQ.c2_digit_stride = z.dQ; KQ.c2_poly_stride = z.sQ;
    KQ.out0 = acc.p[0] + m0 * acc.stride[0]; KQ.out1 = acc.p[1] + m0 * acc.stride[1]; KQ.out_stride = acc.stride[0]; KQ.out1_stride = acc.stride[1];
    KQ.lp = cQ->d_lp;
    KQ.wide = keymac_wide_ok(pl, cQ, z.beta) ? 1 : 0;
    KQ.own = dig.own ? dig.own + m0 * dig.own_stride : nullptr; KQ.own_stride = dig.own_stride; KQ.alpha = dig.own ? pl->dec->alpha : 0;
    const KeyMacLaunch KP = keymac_p_part(pl, KQ, z, dig.P + m0 * z.sP, pl->poolPP.d + m0 * z.sP, pl->poolPP.d + ((long long)batch + m0) * z.sP);
    // a small batch: the Q part and the P part as one launch (they share nothing and each is a few hundred workgroups)
    hipError_t pe = hipErrorNotSupported;
    if (!pl->opt.no_pair && (long long)members * (level + 1) <= pl->opt.pair_max_workgroups) pe = launch_keymac_pair(KQ, level + 1, KP, nP, members, cQ->stream);
    if (pe == hipErrorNotSupported) {
        LR_HIP(launch_keymac(KQ, level + 1, members, cQ->stream));
        LR_HIP(launch_keymac(KP, nP, members, cQ->stream));
    } else if (pe != hipSuccess) {
        return fail(LR_ERR_HIP, std::string("launch_keymac_pair: ") + hipGetErrorString(pe));
    }
    return LR_OK;
}

// bfv.switchKeys' tail (bfv/evaluator.go:806-811): InvNTT over Q||P, then ModDownPQ in the coefficient domain (in place: the extension
// reads x where it stores, ExtSegment::epi_mode 1).  acc / pl->poolPP as ks_inner_product left them.
int ks_coeff_tail(lr_ckks_plan *pl, int level, int batch, const KeySwitchAcc &acc) {
    lr_context *cQ = pl->cQ, *cP = pl->cP;
    lr_bext *bx = pl->bext;
    const int nP = cP->h.L(), n = (int)cQ->h.N;
    const KsSizes z = ks_sizes(pl, level, batch);
    u64 *const poolP[2] = {pl->poolPP.d, pl->poolPP.d + z.dP};
    const Rows pr{poolP[0], z.sP, 0, 1};
    // the two accumulators as ONE batch where they can be (the relinearisation's pool lies back to back; one poly each at any distance)
    const ComponentPair both = component_pair(acc.p[0], acc.stride[0], acc.p[1], acc.stride[1], batch);
    const bool pair = !pl->opt.no_pair && both;
    if (pair) {
        const Rows qr{acc.p[0], both.stride, 0, 1};
        LR_TRY(run_ntt(cQ, true, qr, qr, 0, 1, level + 1, 2 * batch));
    } else {
        for (int k = 0; k < 2; ++k) {
            const Rows qr{acc.p[k], acc.stride[k], 0, 1};
            LR_TRY(run_ntt(cQ, true, qr, qr, 0, 1, level + 1, batch));
        }
    }
    LR_TRY(run_ntt(cP, true, pr, pr, 0, 1, nP, 2 * batch));
    const bool fused = !cQ->opt.no_epilogue && ext_epilogue_supported(bx->pq.tables(), nP, n);
    auto moddown = [&](u64 *x, long long x_stride, const Rows &p, int polys) -> int {
        if (!fused) {
            LR_TRY(bx->poolQ.ensure(cQ, (size_t)polys * z.sQ));
            LR_TRY(run_ext(cQ, bx->pq, nP, p, polys, segment(bx->poolQ.d, z.sQ, 0, 0, level + 1), segment(nullptr, 0, 0, 0, 0)));
            return run_submul(cQ, level + 1, polys, x, x_stride, bx->poolQ.d, z.sQ, (long long)n, x, x_stride, bx->d_moddown_pq, false, nullptr);
        }
        ExtSegment sd = segment(x, x_stride, 0, 0, level + 1);
        sd.epi_mode = 1;
        sd.epi_x = x;
        sd.epi_x_stride = x_stride;
        sd.epi_c = bx->d_moddown_pq;
        return run_ext(cQ, bx->pq, nP, p, polys, sd, segment(nullptr, 0, 0, 0, 0));
    };
    if (pair && fused) return moddown(acc.p[0], both.stride, pr, 2 * batch);      // (the two halves of poolPP lie back to back)
    for (int k = 0; k < 2; ++k) LR_TRY(moddown(acc.p[k], acc.stride[k], Rows{poolP[k], z.sP, 0, 1}, batch));
    return LR_OK;
}

// ModDownSplitedNTTPQ x2 (:1537-1557 / :1367-1387); the two calls share every launch up to the final subtract-multiply.
// acc / pl->poolPP as ks_inner_product left them; without `fin` (plain SwitchKeysInPlace) the results replace acc and nothing is added.
int ks_ntt_tail(lr_ckks_plan *pl, int level, int batch, const KeySwitchAcc &acc, const KeySwitchEpilogue *fin) {
    lr_context *cQ = pl->cQ, *cP = pl->cP;
    lr_bext *bx = pl->bext;
    const int nP = cP->h.L(), n = (int)cQ->h.N;
    const long long n64 = (long long)n;
    const KsSizes z = ks_sizes(pl, level, batch);
    const long long sQ = z.sQ;
    // the two components: x - ext goes, times the ModDown constant and plus the addend, to out
    struct Component {
        const u64 *x;
        u64 *out;
        const u64 *plus;      // nullptr: none (the rotations' second component)
        long long x_stride, out_stride, plus_stride;
    };
    const Component comp[2] = {
        {acc.p[0], fin ? fin->out0 : acc.p[0], fin ? fin->plus0 : nullptr, acc.stride[0], fin ? fin->out_stride : acc.stride[0], fin ? fin->plus_stride : 0},
        {acc.p[1], fin ? fin->out1 : acc.p[1], fin ? fin->plus1 : nullptr, acc.stride[1],
         fin ? (fin->out1_stride ? fin->out1_stride : fin->out_stride) : acc.stride[1], fin ? (fin->plus1_stride ? fin->plus1_stride : fin->plus_stride) : 0}};
    const Rows pr{pl->poolPP.d, z.sP, 0, 1};
    LR_TRY(bx->poolQ.ensure(cQ, (size_t)2 * batch * sQ));
    u64 *ext_out = bx->poolQ.d;
    const bool asm16 = cQ->h.logN == 16 && cQ->use_asm && cQ->asm_fwd >= 0;
    const bool asm15 = cQ->h.logN == 15 && ntt_split15(cQ, (long long)(level + 1) * batch);     // (one launch per component)
    const bool exttop = (asm16 || asm15) && !pl->opt.no_exttop && ext_top_supported(bx->pq.tables(), nP, n);
    if (asm16 && !exttop && !pl->opt.no_staging) {
        LR_TRY(pl->stageQ.ensure(cQ, (size_t)2 * batch * sQ));     // (the digits' staging area is free again)
        ext_out = pl->stageQ.d;
    }
    ExtSegment mseg = segment(ext_out, sQ, 0, 0, level + 1);
    if (exttop) mseg.top_tw = cQ->d_fwd;                           // the ModDown transform's top stage inside the extension
    // ... and the last stage of the inverse transform in front of it (see ks_plan_decomposition)
    const bool invtop = exttop && !pl->opt.no_invtop && cP->asm_inv >= 0 && bx->pq.invtop0 != nullptr && nP <= 8;
    LR_TRY(run_ntt(cP, true, pr, pr, 0, 1, nP, 2 * batch, 0, 0, nullptr, false, invtop));
    LR_TRY(run_ext(cQ, bx->pq, nP, pr, 2 * batch, mseg, segment(nullptr, 0, 0, 0, 0), nullptr, nullptr, invtop));
    // limbs [l0, l1): both components' forward transform in one launch, then the separate subtract-multiply passes
    auto transform_then_submul = [&](int l0, int l1) -> int {
        LR_TRY(run_ntt(cQ, false, Rows{ext_out, sQ, l0, 1}, Rows{bx->poolQ.d, sQ, l0, 1}, l0, 1, l1 - l0, 2 * batch, 0, 0, nullptr, exttop));
        for (int k = 0; k < 2; ++k) {
            const Component &c = comp[k];
            LR_TRY(run_submul(cQ, l1 - l0, batch, c.x + l0 * n64, c.x_stride, bx->poolQ.d + (long long)k * batch * sQ + l0 * n64, sQ, n64, c.out + l0 * n64,
                              c.out_stride, bx->d_moddown_pq + l0, false, nullptr, c.plus ? c.plus + l0 * n64 : nullptr, c.plus_stride, nullptr, l0));
        }
        return LR_OK;
    };
    if (!ntt_epilogue_ok(cQ)) return transform_then_submul(0, level + 1);
    // the subtract-multiply and the addition of MulRelin / the rotations inside the forward transform's copy-out, for
    // every run of limbs below 2^46 (FP64 body); the other limbs keep the separate pass
    if ((!comp[0].plus || !comp[1].plus) && pl->zerosQ.words < (size_t)sQ) {
        LR_TRY(pl->zerosQ.ensure(cQ, (size_t)sQ));
        LR_HIP(hipMemsetAsync(pl->zerosQ.d, 0, (size_t)sQ * sizeof(u64), cQ->stream));
    }
    // (a component without an addend adds the row of zeros)
    const NttEpilogue ep[2] = {
        {comp[0].x, comp[0].x_stride, comp[0].plus ? comp[0].plus : pl->zerosQ.d, comp[0].plus ? comp[0].plus_stride : 0, bx->d_moddown_pq_epi},
        {comp[1].x, comp[1].x_stride, comp[1].plus ? comp[1].plus : pl->zerosQ.d, comp[1].plus ? comp[1].plus_stride : 0, bx->d_moddown_pq_epi}};
    // one ciphertext: the two components as a batch of two whose strides are the distances between their operands (ext_out holds them
    // back to back; x, plus and the outputs are separate allocations) -- one launch instead of two
    const ComponentPair outs = component_pair(comp[0].out, comp[0].out_stride, comp[1].out, comp[1].out_stride, batch);
    const bool pair = batch == 1 && !pl->opt.no_pair && outs;
    for (int l0 = 0, l1; l0 <= level; l0 = l1) {
        bool fpc;
        l1 = epilogue_run_end(cQ, l0, level + 1, &fpc);
        if (!fpc) {
            LR_TRY(transform_then_submul(l0, l1));
        } else if (pair) {
            const NttEpilogue both{ep[0].x, component_distance(ep[0].x, ep[1].x), ep[0].plus, component_distance(ep[0].plus, ep[1].plus), ep[0].consts};
            LR_TRY(run_ntt(cQ, false, Rows{ext_out, sQ, l0, 1}, Rows{comp[0].out, outs.stride, l0, 1}, l0, 1, l1 - l0, 2, 0, 0, &both, exttop));
        } else {
            // the two components are independent launches: side by side while one alone leaves most of the chip idle
            PlanFork fork1(pl, (l1 - l0) * batch);
            LR_TRY(fork1.rc);
            for (int k = 1; k >= 0; --k) {
                LR_TRY(run_ntt(cQ, false, Rows{ext_out + (long long)k * batch * sQ, sQ, l0, 1}, Rows{comp[k].out, comp[k].out_stride, l0, 1}, l0, 1, l1 - l0, batch,
                               0, 0, &ep[k], exttop));
                fork1.back();
            }
            LR_TRY(fork1.join());
        }
    }
    return LR_OK;
}

// the inner product and the NTT-domain tail: what follows the decomposition in every CKKS key switch
int ks_product_and_ntt_tail(lr_ckks_plan *pl, int level, int batch, const KsDigits &dig, const lr_poly *evk, const KeySwitchAcc &acc, const KeySwitchEpilogue *fin) {
    LR_TRY(ks_inner_product(pl, level, batch, dig, evk, acc));
    return ks_ntt_tail(pl, level, batch, acc, fin);
}

}  // namespace

// switchKeysInPlace, ckks/evaluator.go:1475-1558, on raw buffers
int switch_keys_core(lr_ckks_plan *pl, int level, int batch, const u64 *cx, long long cx_stride, const lr_poly *evk, const KeySwitchAcc &acc,
                     const KeySwitchEpilogue *fin) {
    LR_TRY(ks_decompose(pl, level, batch, cx, cx_stride, KsInput::Ntt));
    return ks_product_and_ntt_tail(pl, level, batch, KsDigits::in_place(pl, cx, cx_stride), evk, acc, fin);
}

int check_ct(const lr_ckks_plan *pl, int level, const lr_poly *p, int batch) {
    if (!p) return fail(LR_ERR_ARG, "null poly");
    if (p->N != pl->cQ->h.N) return fail(LR_ERR_SHAPE, "ring degree mismatch");
    if (p->limbs < level + 1) return fail(LR_ERR_SHAPE, "poly has fewer limbs than level+1");
    if (p->batch != batch) return fail(LR_ERR_SHAPE, "batch mismatch");
    return LR_OK;
}

// The checks the pipelines' entry points share (here and in lr_abi_bfv_eval.cpp), after their null checks.  The first that fails decides
// the code a doubly wrong call gets, so each entry point keeps the order it always had: most are check_call; lr_bfv_switch_keys and
// lr_bfv_relinearize ask in another.
int check_batch(const lr_ckks_plan *pl, int batch) {
    if (batch > pl->max_batch) return fail(LR_ERR_SHAPE, "batch exceeds the plan's max_batch");
    return LR_OK;
}
int check_cts(const lr_ckks_plan *pl, int level, int batch, std::initializer_list<const lr_poly *> cts) {
    for (const lr_poly *p : cts) LR_TRY(check_ct(pl, level, p, batch));
    return LR_OK;
}
int check_call(const lr_ckks_plan *pl, int level, int batch, std::initializer_list<const lr_poly *> cts) {
    if (level < 0 || level + 1 > pl->cQ->h.L()) return fail(LR_ERR_SHAPE, "level out of range");
    LR_TRY(check_batch(pl, batch));
    return check_cts(pl, level, batch, cts);
}
// a pipeline that interleaves launches of both contexts: they must be on one stream; the plan's device becomes current
int begin_pipeline(const lr_ckks_plan *pl) {
    LR_TRY(same_stream(pl->cQ, pl->cP));
    LR_HIP(hipSetDevice(pl->device));
    return LR_OK;
}

}  // namespace lr_host

extern "C" int lr_ckks_switch_keys(lr_ckks_plan *pl, int level, const lr_poly *cx, const lr_poly *evk, lr_poly *p0, lr_poly *p1) {
    return guarded([&]() -> int {
    if (!pl || !cx || !evk || !p0 || !p1) return fail(LR_ERR_ARG, "null argument");
    const int batch = cx->batch;
    LR_TRY(check_call(pl, level, batch, {cx, p0, p1}));
    LR_TRY(begin_pipeline(pl));
    return switch_keys_core(pl, level, batch, cx->d, cx->stride(), evk, {{p0->d, p1->d}, {p0->stride(), p1->stride()}});
    });
}

// bfv.evaluator.switchKeys (bfv/evaluator.go:736-812): cx in the coefficient domain over all of Q, evk over Q||P in the NTT +
// Montgomery domain like the reference's SwitchingKey; p0 / p1 <- the two key-switched polys over Q, coefficient domain.  Same
// machinery as the CKKS key switch (one plan over contextQ / contextP serves both), with the transforms the other way round.
int lr_host::bfv_switch_keys_core(lr_ckks_plan *pl, int batch, const u64 *cx, long long cx_stride, const lr_poly *evk, const KeySwitchAcc &acc) {
    return bfv_switch_keys_grouped(pl, batch, 1, cx, cx_stride, &evk, acc);
}

// `groups` independent bfv.switchKeys of `batch` polys each as ONE pass over groups * batch members (lr_bfv_relinearize_deg: the key
// switches of ct[degree], ct[degree - 1], ... share no data): member g * batch + b of cx and of the accumulators is poly b of group g,
// switched under evks[g].  Decomposition and tail run once over all members; only the inner product is per key, on its group's member
// range.  Every member gets the bits of a key switch of its own.
int lr_host::bfv_switch_keys_grouped(lr_ckks_plan *pl, int batch, int groups, const u64 *cx, long long cx_stride, const lr_poly *const *evks,
                                     const KeySwitchAcc &acc) {
    const int level = pl->cQ->h.L() - 1, members = groups * batch;
    LR_TRY(ks_decompose(pl, level, members, cx, cx_stride, KsInput::Coeff));
    const long long sQ = (long long)pl->cQ->h.L() * (long long)pl->cQ->h.N;
    for (int g = 0; g < groups; ++g)
        LR_TRY(ks_inner_product(pl, level, members, KsDigits::in_place(pl, pl->c2.d, sQ), evks[g], acc, groups == 1 ? KsMembers() : KsMembers{g * batch, batch}));
    return ks_coeff_tail(pl, level, members, acc);
}

// RotateHoisted + switchKeyHoisted (ckks/evaluator.go:1252-1391): n_rot rotations of one ciphertext share the
// digit decomposition; per rotation the digits are permuted, multiplied into the rotation key and brought down.
extern "C" int lr_ckks_rotate_hoisted(lr_ckks_plan *pl, int level, const lr_poly *c0, const lr_poly *c1, int n_rot,
                                      const uint64_t *gens, const lr_poly *const *rotkeys, lr_poly *const *outs0,
                                      lr_poly *const *outs1) {
    return guarded([&]() -> int {
    if (!pl || !c0 || !c1 || !gens || !rotkeys || !outs0 || !outs1) return fail(LR_ERR_ARG, "null argument");
    if (n_rot < 0) return fail(LR_ERR_ARG, "negative rotation count");
    const int batch = c0->batch;
    LR_TRY(check_call(pl, level, batch, {c0, c1}));
    lr_context *cQ = pl->cQ, *cP = pl->cP;
    LR_TRY(begin_pipeline(pl));
    const int nP = cP->h.L(), n = (int)cQ->h.N, L1 = level + 1;
    const KsSizes z = ks_sizes(pl, level, batch);
    const int beta = z.beta;
    const long long s = (long long)L1 * n, sQ = z.sQ, sP = z.sP;
    for (int r = 0; r < n_rot; ++r) {
        if (!rotkeys[r] || !outs0[r] || !outs1[r]) return fail(LR_ERR_ARG, "null argument");
        LR_TRY(check_cts(pl, level, batch, {outs0[r], outs1[r]}));
        if (outs0[r]->stride() != outs1[r]->stride()) return fail(LR_ERR_SHAPE, "output polys must share their stride");
        if (outs0[r]->d == c0->d || outs1[r]->d == c0->d || outs0[r]->d == c1->d || outs1[r]->d == c1->d)
            return fail(LR_ERR_ARG, "hoisted rotations are not in place");
    }
    LR_TRY(ks_decompose(pl, level, batch, c1->d, c1->stride(), KsInput::NttCopyOwn));          // :1258-1272
    for (Pool *p : {&pl->c0, &pl->q1, &pl->q2}) LR_TRY(p->ensure(cQ, (size_t)batch * s));
    const KeySwitchAcc acc{{pl->q1.d, pl->q2.d}, {s, s}};
    if (pl->opt.no_epilogue) {
        LR_TRY(pl->permQ.ensure(cQ, (size_t)beta * batch * sQ));
        LR_TRY(pl->permP.ensure(cQ, (size_t)beta * batch * sP));
    }
    for (int r = 0; r < n_rot; ++r) {
        LR_TRY(run_permute_ntt(cQ, L1, batch, c0->d, c0->stride(), pl->c0.d, s, gens[r]));     // :1314-1318
        KeySwitchEpilogue fin{outs0[r]->d, outs1[r]->d, outs0[r]->stride(), pl->c0.d, nullptr, s};   // :1389-1390
        if (pl->opt.no_epilogue) {
            // the reference's shape: permuted copies of every digit (:1346-1347), then the inner product over them
            LR_TRY(run_permute_ntt(cQ, L1, beta * batch, pl->c2QiQ.d, sQ, pl->permQ.d, sQ, gens[r]));
            LR_TRY(run_permute_ntt(cP, nP, beta * batch, pl->c2QiP.d, sP, pl->permP.d, sP, gens[r]));
            LR_TRY(ks_product_and_ntt_tail(pl, level, batch, KsDigits::whole(pl->permQ.d, pl->permP.d), rotkeys[r], acc, &fin));
        } else {
            // the permutation of the digits rides on the inner product's loads (KeyMacLaunch::perm_gen): same values, 2 x beta x (|Q| + |P|)
            // rows per rotation less to write and read back
            LR_TRY(ks_product_and_ntt_tail(pl, level, batch, KsDigits::whole(pl->c2QiQ.d, pl->c2QiP.d, gens[r]), rotkeys[r], acc, &fin));
        }
    }
    return LR_OK;
    });
}

// pkEncryptor.encrypt, the branch through the special primes, after the sampling (ckks/encryptor.go:205-234).
// u, pk0, pk1, e0, e1 hold |Q|+|P| limbs (the layout of contextQP); pk0 / pk1 may have batch 1.
extern "C" int lr_ckks_encrypt_pk(lr_ckks_plan *pl, int level, const lr_poly *u, const lr_poly *pk0, const lr_poly *pk1,
                                  const lr_poly *e0, const lr_poly *e1, const lr_poly *pt, lr_poly *o0, lr_poly *o1) {
    return guarded([&]() -> int {
    if (!pl || !u || !pk0 || !pk1 || !e0 || !e1 || !pt || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    lr_context *cQ = pl->cQ, *cP = pl->cP;
    const int nQ = cQ->h.L(), nP = cP->h.L(), n = (int)cQ->h.N;
    if (level < 0 || level + 1 > nQ) return fail(LR_ERR_SHAPE, "level out of range");
    const int batch = u->batch;
    if (batch > pl->max_batch) return fail(LR_ERR_SHAPE, "batch exceeds the plan's max_batch");
    for (const lr_poly *p : {u, pk0, pk1, e0, e1}) {
        if (p->N != cQ->h.N || p->limbs < nQ + nP) return fail(LR_ERR_SHAPE, "encrypt: u, pk and e hold |Q|+|P| limbs");
        if (p->batch != batch && !((p == pk0 || p == pk1) && p->batch == 1)) return fail(LR_ERR_SHAPE, "batch mismatch");
    }
    LR_TRY(check_ct(pl, level, o0, batch));
    LR_TRY(check_ct(pl, level, o1, batch));
    if (pt->N != cQ->h.N || pt->limbs < level + 1 || (pt->batch != batch && pt->batch != 1)) return fail(LR_ERR_SHAPE, "plaintext: limbs or batch");
    LR_TRY(same_stream(cQ, cP));
    LR_HIP(hipSetDevice(cQ->device));
    const long long sQP = (long long)(nQ + nP) * n, offP = (long long)nQ * n;
    LR_TRY(pl->encQ.ensure(cQ, (size_t)2 * batch * sQP));
    u64 *const pool[2] = {pl->encQ.d, pl->encQ.d + (long long)batch * sQP};
    const lr_poly *pk[2] = {pk0, pk1}, *e[2] = {e0, e1};
    lr_poly *outs[2] = {o0, o1};
    const bool fused = !pl->opt.no_epilogue;     // Options::no_epilogue: the reference's call-by-call shape (one launch per Context call)
    if (fused) {
        // :209-211 both products with the public key in one pass over u (Q rows under contextQ's moduli, P rows under contextP's)
        Mul2Launch M;
        M.a = u->d; M.a_stride = u->stride();
        M.b0 = pk0->d; M.b0_stride = pk0->batch == 1 && batch > 1 ? 0 : pk0->stride();
        M.b1 = pk1->d; M.b1_stride = pk1->batch == 1 && batch > 1 ? 0 : pk1->stride();
        M.out0 = pool[0]; M.out1 = pool[1];
        M.out0_stride = M.out1_stride = sQP;
        M.n = n;
        M.lp = cQ->d_lp;
        LR_HIP(launch_mul2(M, nQ, batch, cQ->stream));
        M.a += offP; M.b0 += offP; M.b1 += offP; M.out0 += offP; M.out1 += offP;
        M.lp = cP->d_lp;
        LR_HIP(launch_mul2(M, nP, batch, cQ->stream));
    } else {
        for (int k = 0; k < 2; ++k) {
            const long long ks = pk[k]->batch == 1 && batch > 1 ? 0 : pk[k]->stride();
            // :209-211 contextQP.MulCoeffsMontgomery(u, pk[k], pool[k]): the Q rows under contextQ's moduli, the P rows under contextP's
            LR_TRY(run_ewise(cQ, LR_MUL_MONT, nQ, batch, u->d, u->stride(), pk[k]->d, ks, pool[k], sQP, nullptr));
            LR_TRY(run_ewise(cP, LR_MUL_MONT, nP, batch, u->d + offP, u->stride(), pk[k]->d + offP, ks, pool[k] + offP, sQP, nullptr));
        }
    }
    {   // :214-215 contextQP.InvNTT, both polys in one launch per basis
        Rows q{pool[0], sQP, 0, 1}, p{pool[0], sQP, nQ, 1};
        LR_TRY(run_ntt(cQ, true, q, q, 0, 1, nQ, 2 * batch));
        LR_TRY(run_ntt(cP, true, p, p, 0, 1, nP, 2 * batch));
    }
    // the Q rows' share of SampleAndAdd rides in the ModDown's extension epilogue (x = CRed(pool + e) where the extension reads x) when the
    // call is at the top level (below it the reference's ModDownPQ reads rows level+1.. of Q as its "P part": those rows need their e first)
    const bool add_in_ext = fused && level == nQ - 1 && moddown_epilogue_available(pl->bext);
    for (int k = 0; k < 2; ++k) {
        // :218-220 SampleAndAdd: CRed(x + e) per coefficient (ring/gaussianSampler.go:268)
        if (!add_in_ext) LR_TRY(run_ewise(cQ, LR_ADD, nQ, batch, pool[k], sQP, e[k]->d, e[k]->stride(), pool[k], sQP, nullptr));
        LR_TRY(run_ewise(cP, LR_ADD, nP, batch, pool[k] + offP, sQP, e[k]->d + offP, e[k]->stride(), pool[k] + offP, sQP, nullptr));
        // :223-226 ModDownPQ(level, pool[k], ct[k]): the P part is read at rows level+1.. (ring_basis_extension.go:255)
        Rows pP{pool[k], sQP, level + 1, 1};
        LR_TRY(moddown_pq_core(pl->bext, level, pool[k], sQP, pP, batch, outs[k], false, add_in_ext ? e[k]->d : nullptr, e[k]->stride()));
        Rows r = rows_of(outs[k]);
        LR_TRY(run_ntt(cQ, false, r, r, 0, 1, level + 1, batch));                                                     // :229-230
    }
    const long long ps = pt->batch == 1 && batch > 1 ? 0 : pt->stride();
    return run_ewise(cQ, LR_ADD, level + 1, batch, o0->d, o0->stride(), pt->d, ps, o0->d, o0->stride(), nullptr);     // :234
    });
}

// decryptor.Decrypt (ckks/decryptor.go:53-78): Horner evaluation of the ciphertext at the secret key
extern "C" int lr_ckks_decrypt(lr_ckks_plan *pl, int level, const lr_poly *const *ct, int degree, const lr_poly *sk, lr_poly *pt) {
    return guarded([&]() -> int {
    if (!pl || !ct || !sk || !pt) return fail(LR_ERR_ARG, "null argument");
    if (degree < 0) return fail(LR_ERR_ARG, "negative degree");
    lr_context *cQ = pl->cQ;
    if (level < 0 || level + 1 > cQ->h.L()) return fail(LR_ERR_SHAPE, "level out of range");
    const int batch = pt->batch, L1 = level + 1;
    for (int i = 0; i <= degree; ++i) {
        if (!ct[i]) return fail(LR_ERR_ARG, "null argument");
        LR_TRY(check_ct(pl, level, ct[i], batch));
    }
    LR_TRY(check_ct(pl, level, pt, batch));
    if (sk->N != cQ->h.N || sk->limbs < L1 || (sk->batch != batch && sk->batch != 1)) return fail(LR_ERR_SHAPE, "secret key: limbs or batch");
    LR_HIP(hipSetDevice(cQ->device));
    const long long ss = sk->batch == 1 && batch > 1 ? 0 : sk->stride();
    bool aliased = false;      // the fused pass reads every ct[i] where it writes pt: fine for ct[degree] == pt only if nothing else is pt
    for (int i = 0; i < degree; ++i) aliased = aliased || ct[i]->d == pt->d;
    if (degree <= kHornerMaxDegree && !aliased && !pl->opt.no_epilogue) {
        // one pass: every component and the key read once, the plaintext written once (the element operations and the reduction
        // cadence are the reference's, HornerLaunch); Options::no_epilogue keeps the call-by-call form below
        HornerLaunch H;
        std::memset(&H, 0, sizeof H);
        for (int i = 0; i <= degree; ++i) {
            H.ct[i] = ct[i]->d;
            H.ct_stride[i] = ct[i]->stride();
        }
        H.sk = sk->d;
        H.sk_stride = ss;
        H.out = pt->d;
        H.out_stride = pt->stride();
        H.degree = degree;
        H.n = (int)cQ->h.N;
        H.lp = cQ->d_lp;
        LR_HIP(launch_horner(H, L1, batch, cQ->stream));
        return LR_OK;
    }
    LR_TRY(run_ewise(cQ, LR_COPY, L1, batch, ct[degree]->d, ct[degree]->stride(), nullptr, 0, pt->d, pt->stride(), nullptr));   // :61
    for (int i = degree; i > 0; --i) {
        LR_TRY(run_ewise(cQ, LR_MUL_MONT, L1, batch, pt->d, pt->stride(), sk->d, ss, pt->d, pt->stride(), nullptr));            // :67
        LR_TRY(run_ewise(cQ, LR_ADD, L1, batch, pt->d, pt->stride(), ct[i - 1]->d, ct[i - 1]->stride(), pt->d, pt->stride(), nullptr));   // :68
        if ((i & 7) == 7) LR_TRY(run_ewise(cQ, LR_REDUCE, L1, batch, pt->d, pt->stride(), nullptr, 0, pt->d, pt->stride(), nullptr));     // :70
    }
    if ((degree & 7) != 7) LR_TRY(run_ewise(cQ, LR_REDUCE, L1, batch, pt->d, pt->stride(), nullptr, 0, pt->d, pt->stride(), nullptr));    // :75
    return LR_OK;
    });
}
