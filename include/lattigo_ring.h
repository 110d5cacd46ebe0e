/*
 * lattigo_ring.h -- C ABI of the MI355X-native `ring` hot path.
 *
 * This is the drop-in boundary for Lattigo v1.3.1's `ring` package
 * (github.com/ldsec/lattigo/ring).  The reference has no FFI of its own: bfv/ckks
 * call methods on *ring.Context, *ring.FastBasisExtender and *ring.Decomposer
 * directly.  A Go shim package with the same exported identifiers forwards each
 * method to the entry point below that names it (see INTEGRATION.md for the cgo
 * stub).  Every entry point cites the reference symbol it replaces
 * (path:line relative to the Lattigo tree).
 *
 * Conventions
 *  - plain C, opaque handles, pointers and sizes only; no exceptions or aborts cross
 *    the boundary.  Every function returns an lr_status (0 = ok).
 *  - a handle is bound to one HIP device and one HIP stream.  Calls are asynchronous
 *    on that stream unless the name ends in _host or the doc says "synchronises".
 *    Distinct handles may be used from distinct threads; one handle is single-threaded,
 *    like the reference's evaluators (examples/dbfv/psi/psi.go:221).
 *  - lr_poly is a device-resident batch of polynomials laid out (poly, limb, coeff)-major:
 *        coeff(b, i, j) = base[(b * limbs + i) * N + j]          uint64
 *    i.e. the dense image of `batch` Go values `Poly.Coeffs [][]uint64`
 *    (ring/ring_object.go:11-13).  Every operation applies to all polys of the batch;
 *    an operand with batch == 1 is broadcast (shared keys / constants).
 *  - "level" has the reference's meaning: limbs 0..level are touched, the rest ignored
 *    (ring/ntt.go:11, ring/ring.go:20).  Passing more limbs than a poly owns is
 *    LR_ERR_SHAPE (Go would panic with an index error).
 *  - in == out aliasing is legal wherever the reference allows it (everywhere; the Galois permutations are "not in place" in the
 *    reference as well, ring/ring_galois.go:54, and return LR_ERR_ARG).
 *  - results are bit-identical to the reference on the same inputs.
 *  - threads: an lr_context is immutable after creation and may be shared by threads, each with its own polys / extender /
 *    decomposer / plan (the reference's goroutine-per-evaluator model); its temporaries are leased per call.  Every other handle
 *    is single-threaded, like the reference's FastBasisExtender and evaluators (their scratch polys, ring_basis_extension.go:16-17).
 *  - configuration is an lr_options struct handed to the *_create_ex entry points (below); the plain *_create forms use the defaults.
 *    The LR_* environment variables of INTEGRATION.md section 7 are a TEST-ONLY override of the same fields, read in one place
 *    (lr::Options::apply_env) when a handle is created; a deployment sets none of them.
 */
#ifndef LATTIGO_RING_H
#define LATTIGO_RING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum lr_status {
    LR_OK = 0,
    LR_ERR_INVALID_DEGREE = 1, /* N not a power of two: ring/ring_context.go:71-73 (panic in Go)            */
    LR_ERR_NOT_NTT_FRIENDLY = 2, /* "provided modulus does not allow NTT": ring/ring_context.go:141-146     */
    LR_ERR_SHAPE = 3,          /* limb/batch/N mismatch (Go: index-out-of-range panic)                       */
    LR_ERR_ARG = 4,            /* null handle, bad enum, unsupported parameter                               */
    LR_ERR_HIP = 5,            /* HIP runtime failure; see lr_last_error_string()                            */
    LR_ERR_UNSUPPORTED = 6,    /* size outside what the kernels are built for                                */
    LR_ERR_NOMEM = 7,          /* host allocation failed (std::bad_alloc caught at the boundary)                */
    LR_ERR_INTERNAL = 8        /* any other C++ exception caught at the boundary; see lr_last_error_string()    */
} lr_status;

typedef struct lr_context lr_context;       /* ring.Context           ring/ring_context.go:18-51            */
typedef struct lr_poly lr_poly;             /* batch of ring.Poly     ring/ring_object.go:11-13             */
typedef struct lr_bext lr_bext;             /* ring.FastBasisExtender ring/ring_basis_extension.go:9-18     */
typedef struct lr_decomposer lr_decomposer; /* ring.Decomposer        ring/ring_basis_extension.go:398-407  */
typedef struct lr_simple_scaler lr_simple_scaler; /* ring.SimpleScaler  ring/ring_scaling.go:168-181           */
typedef struct lr_ckks_plan lr_ckks_plan;   /* scratch pools + tables of ckks.evaluator, ckks/evaluator.go:63-97 */

const char *lr_last_error_string(void);     /* thread-local, never NULL */
int lr_device_count(int *count);
/* version / build info: "lattigo_ring <ver> gfx950 hip" */
const char *lr_build_info(void);

/* ------------------------------------------------------------------ options ---------- */
/* Every switch selects between code paths that give THE SAME BITS (each has a parity test that runs both); the defaults are the measured
 * best on MI355X.  A caller fills the struct with lr_options_init and changes what it wants; `struct_size` lets a library newer than its
 * caller tell which fields the caller knows (fields beyond struct_size take their defaults), `version` must be LR_OPTIONS_VERSION.
 * Flags: 0 = the default path, non-zero = the alternative the field names.  Thresholds: 0 = the built-in default (in parentheses;
 * measured on PN15QP880 / PN16QP1761 / PN14QP438, DESIGN.md "decision table").  INTEGRATION.md section 7 maps every LR_* test variable
 * to its field. */
#define LR_OPTIONS_VERSION 1
typedef struct lr_options {
    uint32_t struct_size;           /* sizeof(lr_options) as the caller compiled it                                                   */
    uint32_t version;               /* LR_OPTIONS_VERSION                                                                             */
    /* --- transforms (lr_context) */
    int32_t no_asm;                 /* C++ NTT kernels only (lr_ntt.hip) instead of the gfx950 assembly code objects                  */
    int32_t no_fp;                  /* integer butterflies for every modulus (no FP64 body for the limbs below 2^46)                  */
    int32_t ntt_mode;               /* -1 = by modulus size; 0 / 3: a more conservative lazy-correction mode of the C++ kernels       */
    int32_t asm_variant;            /* -1 = by modulus size; 0 / 1: a more conservative integer variant of the assembly kernels       */
    int32_t asm14_1024;             /* N = 2^14: the 1024-thread kernels at every launch size                                         */
    int32_t no_wide14_small;        /* N = 2^14: the 512-thread kernels for small launches too                                        */
    int32_t wide14_max_items;       /* N = 2^14: launches of at most this many transforms use the 1024-thread kernels (256)           */
    int32_t ntt_split15;            /* N = 2^15 as two 2^14 sub-blocks: -1 = launches of at most split15_max_workgroups, 0 never, 1 always */
    int32_t split15_max_workgroups; /* (128)                                                                                          */
    int32_t no_invfuse;             /* N = 2^16 inverse: lazy sub-blocks + a separate last-stage pass instead of the pair-flag kernels */
    int32_t no_grid_padding;        /* assembly launches with the limb count on grid x as it is (not padded to a multiple of eight)   */
    int32_t ntt_stagger;            /* -1 / 0 = off; kilo-clocks per step of a start-up stagger of the first round of workgroups      */
    int32_t ntt_persist;            /* diagnostics builds only (LR_BUILD_DIAG): polys per workgroup of the persistent forward kernels */
    int32_t ntt_timeline;           /* diagnostics builds only: 2^15 launches run the clock-stamping builds (lr_context_timeline)     */
    /* --- epilogues and the rescale (lr_context) */
    int32_t no_epilogue;            /* separate subtract-multiply passes instead of the forward kernels' / extensions' epilogues      */
    int32_t no_int_epilogue;        /* the epilogue on the FP64 bodies only                                                           */
    int32_t rescale_unfused;        /* rounding rescale with explicit shifted copies                                                  */
    int32_t rescale_unpaired;       /* lr_ckks_rescale: the two components one after the other at every batch size                    */
    int32_t pair_max_workgroups;    /* two components of one ciphertext as ONE launch while it has at most this many workgroups (256) */
    /* --- basis extension (lr_bext, lr_decomposer: taken from their first context) */
    int32_t ext_narrow;             /* one Montgomery product per term instead of the 128-bit column sums                             */
    int32_t ext_ieee_div;           /* IEEE division in the float correction instead of the reciprocal + two residual steps           */
    int32_t no_ext_chunks;          /* a small batch's extension as one launch over all target columns                                */
    /* --- key switch and the pipelines built on it (lr_ckks_plan) */
    int32_t no_staging;             /* N = 2^16: in-place forward transforms after the digits' extensions                             */
    int32_t no_exttop;              /* the top transform stage as its own pass instead of inside the extension                        */
    int32_t no_invtop;              /* the inverse transform's last stage as its own pass instead of inside the extension             */
    int32_t no_ext_group;           /* one extension launch per digit instead of one grouped launch                                   */
    int32_t keymac_narrow;          /* one Montgomery product per term in the key inner product                                       */
    int32_t no_pair;                /* a single ciphertext's two components as two launches                                           */
    int32_t no_fork;                /* never run two independent launches of a lone plan side by side on an auxiliary stream          */
    int32_t fork_below_workgroups;  /* fork only while the forked launch has fewer workgroups than this (256)                         */
    /* --- bfv Mul (lr_bfv_plan) */
    int32_t bfv_no_ext_epilogue;    /* SubScalarBigint / MulScalar as separate passes                                                 */
    int32_t bfv_no_gather;          /* never gather the four operand polys of a small batch into one buffer                           */
    int64_t bfv_gather_below;       /* gather while the joint transform has fewer workgroups than this (1536)                         */
    /* --- bfv Encoder (lr_bfv_encoder) */
    int32_t bfv_encoder_unfused;    /* scatter / InvNTT / lift and scale / NTT / gather as separate launches where the fused kernels would run */
    /* --- ckks Encoder (lr_ckks_encoder) */
    int32_t ckks_encoder_tiled;     /* the tiled route (streaming stages + LDS tiles) where the fused kernels would run (slots <= 2^13) */
} lr_options;
/* fills *opt with the defaults (struct_size = sizeof(lr_options) of THIS library, version = LR_OPTIONS_VERSION) */
int lr_options_init(lr_options *opt);
/* the options a handle ended up with, after the test-only environment override (diagnostics; struct_size / version of the library) */
int lr_context_get_options(const lr_context *ctx, lr_options *out);

/* ------------------------------------------------------------------ Context ---------- */
/* ring.NewContextWithParams = SetParameters + GenNTTParams (ring/ring_context.go:60,68,129).
 * Computes every constant and psi table on the host exactly as the reference does
 * (incl. primitiveRoot's search order, ring/utils.go:182) and uploads them to `device`. */
int lr_context_create(uint64_t N, const uint64_t *moduli, int n_moduli, int device, lr_context **out);
/* the same with explicit options (NULL = defaults).  LR_ERR_ARG for a version this library does not know. */
int lr_context_create_ex(uint64_t N, const uint64_t *moduli, int n_moduli, int device, const lr_options *opt, lr_context **out);
int lr_context_destroy(lr_context *ctx);
/* diagnostics: the assembly NTT variant the context's moduli select (forward, inverse): 0..2 = integer lazy-correction modes,
 * 3 = dual kernels (FP64 butterflies for the limbs below 2^46, integer body for the others), -1 = C++ kernels only */
int lr_context_ntt_variants(const lr_context *ctx, int *forward, int *inverse);
/* use an externally owned hipStream_t; NULL = the library's own stream of that device (a non-blocking stream every context of the
 * device shares by default).  NULL does NOT mean HIP's legacy default stream: handle 0 cannot be expressed here, and the library's
 * stream does not synchronise with the legacy stream -- a caller whose other work (e.g. a framework's collectives) is ordered on
 * its "current" stream must create an explicit stream, make it current and pass its handle (bench.py's config-5 leg).
 * A stream belongs to a CONTEXT; polys, extenders, decomposers and plans run on the stream their contexts have at call time.
 * Handles built over two contexts (lr_bext, lr_ckks_plan, lr_bfv_plan) interleave launches of both: set the same stream on both
 * contexts, or the pipeline entry points return LR_ERR_ARG.  Switching is ordered on the device: the new stream waits for an
 * event recorded on the old one (work already enqueued, and the scratch later calls reuse, stay in order); change streams between
 * calls, not while another thread is inside a call on this context.  THE OLD STREAM MUST STILL BE ALIVE when the switch is made: a
 * caller that owns the stream calls lr_context_set_stream(ctx, NULL) (or installs its next stream) BEFORE destroying it -- recording
 * an event on a destroyed hipStream_t is a use-after-free inside the HIP runtime (it crashes, it does not return an error; measured in
 * round 4), so the library cannot detect it.  If the runtime does report an error for the old stream, the library drains the device
 * instead and installs the new stream all the same.
 * HIP graphs: a pipeline call captured after one warm-up call bakes the addresses of the context's pooled scratch into the graph;
 * the pool never frees a buffer while the context lives, so replays stay valid until lr_context_destroy. */
int lr_context_set_stream(lr_context *ctx, void *hip_stream);
/* diagnostics: name of the kernel the last NTT / InvNTT launch of this context dispatched, e.g. "lr_ntt_fwd15_m1" (assembly
 * code object) or "ntt_fwd_kernel<15>" (C++ kernel); bench.py reports it next to the roofline figures */
int lr_context_last_ntt_kernel(const lr_context *ctx, char *buf, size_t capacity);
/* diagnostics: a context created with LR_NTT_TIMELINE=1 runs its forward N = 2^15 launches of the 60-bit integer kernel on a
 * build of the same kernel that stamps the shader clock (low word of s_memtime) at 13 phase boundaries in every wave.  Copies
 * the stamps of the last such launch to dst: [workgroup = poly * limbs + limb][wave 0..15][16] uint32 (tools/timeline.py names
 * the phases).  dst == NULL: only *count (words needed).  Synchronises.  The transform's results are unchanged. */
int lr_context_timeline(lr_context *ctx, uint32_t *dst, size_t capacity, size_t *count);
/* Diagnostics: the basis extension divides float64(y_i) by float64(q_i) (ring/ring_basis_extension.go:372) with a reciprocal from the
 * host and two residual corrections instead of the generic IEEE expansion; this runs both on `samples` pseudo-random and adversarial
 * operand pairs on the device and counts the quotients that differ in any bit (must be 0). */
int lr_selftest_division(lr_context *ctx, uint64_t samples, uint64_t seed, uint64_t *mismatches);
int lr_context_sync(lr_context *ctx);       /* hipStreamSynchronize on the context's stream */
int lr_context_info(const lr_context *ctx, uint64_t *N, int *n_moduli, int *device);

/* Read-back of the precomputed constants, for parity tests; mirrors the getters
 * GetBredParams/GetMredParams/GetPsi/GetPsiInv/GetNttPsi/GetNttPsiInv/GetNttNInv
 * (ring/ring_context.go:253-285).  dst is host memory of the stated element count. */
typedef enum lr_table {
    LR_TAB_MODULUS = 0,    /* [L]                                  */
    LR_TAB_BRED = 1,       /* [L][2] = {hi, lo} of floor(2^128/q)  */
    LR_TAB_MRED = 2,       /* [L]    q^-1 mod 2^64                 */
    LR_TAB_PSI_MONT = 3,   /* [L]                                  */
    LR_TAB_PSI_INV_MONT = 4, /* [L]                                */
    LR_TAB_NTT_PSI = 5,    /* [L][N] bit-reversed, Montgomery form */
    LR_TAB_NTT_PSI_INV = 6,/* [L][N]                               */
    LR_TAB_NTT_N_INV = 7,  /* [L]                                  */
    LR_TAB_RESCALE = 8,    /* [L][L] row j-1, col i (i<j): rescaleParams[j-1][i], ring_context.go:148-158 */
    LR_TAB_MASK = 9        /* [L]                                  */
} lr_table;
int lr_context_get_table(const lr_context *ctx, int which, uint64_t *dst, size_t dst_count);

/* ------------------------------------------------------------------ Poly ------------- */
/* Context.NewPoly / NewPolyLvl (ring/ring_context.go:288,300), for `batch` polys at once; zero-filled. */
int lr_poly_alloc(lr_context *ctx, int limbs, int batch, lr_poly **out);
/* wrap caller-owned device memory (e.g. a torch uint64/int64 tensor) without copying */
int lr_poly_wrap(lr_context *ctx, void *device_ptr, int limbs, int batch, lr_poly **out);
/* the same with `poly_stride_words` uint64 elements between consecutive polys (>= limbs * N): a component of an array of
 * ciphertexts laid out [ciphertext][component][limb][N] is one lr_poly with the stride of a whole ciphertext */
int lr_poly_wrap_strided(lr_context *ctx, void *device_ptr, int limbs, int batch, long long poly_stride_words, lr_poly **out);
int lr_poly_free(lr_poly *p);
int lr_poly_info(const lr_poly *p, uint64_t *N, int *limbs, int *batch, void **device_ptr);
/* Go boundary: gather from / scatter to the per-limb slices of one Poly ([][]uint64 cannot be
 * passed through cgo as a whole; the shim passes `limbs` pinned *uint64).  Synchronises. */
int lr_poly_upload(lr_poly *p, int batch_index, const uint64_t *const *limb_ptrs, int limbs);
int lr_poly_download(const lr_poly *p, int batch_index, uint64_t *const *limb_ptrs, int limbs);
/* the same one limb at a time (`limb` < the poly's limb count): what a cgo caller under the reference's go 1.13 uses -- a Go slice's
 * pointer may cross for the duration of a call, an array of such pointers in C memory may not (go/ring/poly.go).  Synchronises. */
int lr_poly_upload_limb(lr_poly *p, int batch_index, int limb, const uint64_t *src);
int lr_poly_download_limb(const lr_poly *p, int batch_index, int limb, uint64_t *dst);
/* Poly.MarshalBinary / UnmarshalBinary image of ONE poly (ring/ring_object.go:159-176,222-229,252-270): byte 0 = log2 N,
 * byte 1 = number of moduli, then limb-major big-endian uint64 (WriteCoeffsTo :146, DecodeCoeffs :197).  The bytes
 * cross PCIe as they are and are swapped on the device, so serialized ciphertexts and keys go disk -> HBM without
 * a host pass.  An encoding with fewer moduli than the poly fills its first rows.  Synchronises. */
int lr_poly_unmarshal(lr_poly *p, int batch_index, const uint8_t *data, size_t len);
int lr_poly_marshal(const lr_poly *p, int batch_index, uint8_t *data, size_t capacity, size_t *written);
/* dense host image [batch][limbs][N].  Synchronises. */
int lr_poly_upload_dense(lr_poly *p, const uint64_t *host, size_t count);
int lr_poly_download_dense(const lr_poly *p, uint64_t *host, size_t count);
int lr_poly_zero(lr_poly *p);               /* Poly.Zero, ring/ring_object.go:60 */
/* Rescale re-slices its argument (`p0.Coeffs = p0.Coeffs[:level]`, ring/ring_scaling.go:33);
 * the device buffer keeps its stride, only the logical limb count changes. */
int lr_poly_set_limbs(lr_poly *p, int limbs);

/* ------------------------------------------------------------------ NTT -------------- */
/* Context.NTTLvl / Context.NTT (ring/ntt.go:11,4): forward negacyclic NTT of limbs 0..level of
 * every poly in the batch; natural order in, bit-reversed order out, canonical output [0,q).
 * Accepts any uint64 input the reference accepts (values >= q, see ring/ring_scaling.go:19,102). */
int lr_ntt(lr_context *ctx, int level, const lr_poly *in, lr_poly *out);
/* Context.InvNTTLvl / Context.InvNTT (ring/ntt.go:25,18). */
int lr_intt(lr_context *ctx, int level, const lr_poly *in, lr_poly *out);
/* package-level ring.NTT / ring.InvNTT on ONE limb under modulus index `mod_index`
 * (ring/ntt.go:53,89): in/out limb index select rows of the polys.  Used by callers that
 * transform a foreign limb under another limb's modulus (ring/ring_scaling.go:19,105). */
int lr_ntt_limb(lr_context *ctx, int mod_index, const lr_poly *in, int in_limb, lr_poly *out, int out_limb);
int lr_intt_limb(lr_context *ctx, int mod_index, const lr_poly *in, int in_limb, lr_poly *out, int out_limb);
/* literal drop-in for a Go `Context.NTT(p1, p2)` call on host slices: upload, transform,
 * download.  Synchronises. */
int lr_ntt_host(lr_context *ctx, int level, const uint64_t *const *in_limbs, uint64_t *const *out_limbs);
int lr_intt_host(lr_context *ctx, int level, const uint64_t *const *in_limbs, uint64_t *const *out_limbs);
/* package-level ring.NTT / ring.InvNTT (ring/ntt.go:53,89) on one limb under modulus `mod_index`, host slices, may be in place */
int lr_ntt_host_limb(lr_context *ctx, int mod_index, int inverse, const uint64_t *in, uint64_t *out);

/* ------------------------------------------------------------------ coefficient-wise -- */
/* One entry point for the whole ring/ring.go family; `op` selects the method. */
typedef enum lr_ewise_op {
    LR_ADD = 0,                 /* Add/AddLvl                       ring/ring.go:10,20   */
    LR_ADD_NOMOD = 1,           /* AddNoMod/AddNoModLvl             :32,42               */
    LR_SUB = 2,                 /* Sub/SubLvl                       :54,64               */
    LR_SUB_NOMOD = 3,           /* SubNoMod/SubNoModLvl             :77,87               */
    LR_NEG = 4,                 /* Neg/NegLvl                       :100,110             */
    LR_REDUCE = 5,              /* Reduce/ReduceLvl                 :122,133             */
    LR_MUL_COEFFS = 6,          /* MulCoeffs (Barrett)              :187                 */
    LR_MUL_COEFFS_AND_ADD = 7,  /* MulCoeffsAndAdd                  :198                 */
    LR_MUL_COEFFS_AND_ADD_NOMOD = 8, /* MulCoeffsAndAddNoMod        :209                 */
    LR_MUL_COEFFS_CONSTANT = 9, /* MulCoeffsConstant                :335                 */
    LR_MUL_MONT = 10,           /* MulCoeffsMontgomery(Lvl)         :221,233             */
    LR_MUL_MONT_AND_ADD = 11,   /* MulCoeffsMontgomeryAndAdd(Lvl)   :247,259             */
    LR_MUL_MONT_AND_ADD_NOMOD = 12, /* ...AndAddNoMod(Lvl)          :273,285             */
    LR_MUL_MONT_CONSTANT_AND_ADD_NOMOD = 13, /* ...ConstantAndAddNoModLvl :297           */
    LR_MUL_MONT_AND_SUB = 14,   /* MulCoeffsMontgomeryAndSub        :311                 */
    LR_MUL_MONT_AND_SUB_NOMOD = 15, /* ...AndSubNoMod               :323                 */
    LR_MUL_MONT_CONSTANT = 16,  /* MulCoeffsMontgomeryConstant      :347                 */
    LR_MFORM = 17,              /* MForm/MFormLvl                   :583,595             */
    LR_INV_MFORM = 18,          /* InvMForm                         :610                 */
    LR_MUL_SCALAR = 19,         /* MulScalar/MulScalarLvl           :513,526  scalars[0]            */
    LR_MUL_SCALAR_LIMBS = 20,   /* MulScalarBigint(Lvl)             :541,557  scalars[i] = s mod qi */
    LR_ADD_SCALAR_LIMBS = 21,   /* AddScalarBigint                  :477      (writes its 1st arg)  */
    LR_SUB_SCALAR_LIMBS = 22,   /* SubScalarBigint                  :500      (writes its 1st arg)  */
    LR_COPY = 23,               /* Copy/CopyLvl                     ring/ring_object.go:85,98       */
    LR_MUL_BY_POW2 = 24,        /* MulByPow2/MulByPow2Lvl           ring/ring.go:629,645 scalars[0] */
    LR_EWISE_OP_COUNT = 25
} lr_ewise_op;
/* out <- op(a, b) (accumulating ops read out as well).  b may be NULL for 2-operand ops.
 * scalars: host pointer, 1 value (MUL_SCALAR, MUL_BY_POW2) or level+1 values (*_LIMBS). */
int lr_ewise(lr_context *ctx, int op, int level, const lr_poly *a, const lr_poly *b, lr_poly *out,
             const uint64_t *scalars);

/* ------------------------------------------------------------------ Galois automorphisms */
/* The constant-by-ciphertext methods of ckks.Evaluator index Coeffs directly with one scalar for the coefficients below N/2 and one
 * for the rest (AddConst ckks/evaluator.go:429-445, MultByConstAndAdd :588-606, MultByConst :712-730, MultByi :765-779, DivByi
 * :814-828): out[i][j] = OP(in[i][j], j < N/2 ? lo[i] : hi[i]) for the limbs 0..level, with the reference's exact element operation,
 * op 0: CRed(x + s)   op 1: MRed(x, s)   op 2: CRed(out + MRed(x, s)).  lo / hi: level+1 host words each (the scalars as the
 * reference computes them: scaleUpExact + MForm, or nttPsi[i][1] and its negation).  in may be out. */
int lr_half_scalar_op(lr_context *ctx, int op, int level, const lr_poly *in, const uint64_t *lo, const uint64_t *hi, lr_poly *out);

/* ------------------------------------------------------------------ CKKS linear combination by constants */
/* res = c0 + sum_k c_k ct_k over ciphertexts of degree 1: evaluatePolyFromPowerBasis (ckks/polynomial_evaluation.go:142-159), the leaf
 * of recurse / recurseCheby and of anything that sums ciphertexts weighted by constants.  The reference runs
 *     if has_const:  AddConst(res, c0, res)                 ckks/evaluator.go:373-444
 *     for k = 0 .. n_terms-1, IN THE CALLER'S ORDER:
 *                    MultByConstAndAdd(ct_k, c_k, res)      :451-608, with MultByConst :622-734 where it calls it (:530, :553)
 * (it iterates a Go map there, so its own order -- and with it its output bits, because every step may rescale the receiver -- is
 * random; the caller of these two entry points fixes one).  The chain is split into its scalar lines and its element loops.
 *
 * lr_ckks_lincomb_constants: the scalar lines (everything outside the `for j` / `for u` loops), literally.  HOST ONLY: no context, no
 * device, thread-safe.  Constants are complex128 (re, im); the reference's float64 / uint64 / int64 / int cases are im = 0 with the
 * same arithmetic.
 *   in : moduli[n_moduli] and ntt_psi1[n_moduli] = the word GetNttPsi()[i][1] of each (lr_context_get_table NTT_PSI, entry 1);
 *        default_scale = ckksContext.scale; the receiver's res_level / res_scale before the chain; has_const and c0; per term
 *        term_re / term_im / term_scale / term_level [n_terms].
 *   out: *level_after = min(res_level, every term_level) (DropLevel :457-460), *scale_after; with has_const add_lo / add_hi
 *        [level_after+1]; has_pre[n_terms]; pre / lo / hi [n_terms][level_after+1], rows level_after+1 words apart.  pre[k] is the
 *        Montgomery-form multiplier of the RECEIVER where the reference calls MultByConst(ctOut, ...) at :530 or :553 (has_pre[k] = 1;
 *        real-valued, one word per limb; otherwise the row is zero); lo[k] / hi[k] are scaledConst after MForm for the coefficients
 *        below / above N/2 (:585, :597); add_lo / add_hi are AddConst's scaledConst (:426, :437; no MForm).
 *   DropLevel only lowers the receiver's level and the limbs above the final level are dropped, so words are produced for the limbs
 *   0..level_after only, whatever level a step ran at: equivalent for the limbs that remain.
 *   scaleUpExact (ckks/utils.go:22-49) is restated exactly: 53-bit products and a + 0.5 that rounds to even, truncation, and q itself
 *   for a negative multiple of q.
 *   QUIRK kept: :553 passes a float64 ratio to MultByConst; with a fractional part that call scales the ratio by the default scale
 *   (:656-667) and the scale it sets (:733) is overwritten at :556 -- the receiver is then off by the default scale, as in the
 *   reference.  The lines as they stand (as lr_ckks_encrypt_pk does below the top level).
 *   Domain (Go's float-to-integer conversions are machine-specific out of range): finite constants with |re|, |im| < 2^63, finite
 *   positive scales, every ratio the reference converts with uint64(...) below 2^63, every product constant * scale finite; moduli
 *   odd, in [3, 2^61), each root word below its modulus; levels inside the moduli.  Outside it: LR_ERR_ARG and NOTHING is written.
 *   Checked in this order, messages "CKKS linear combination constants: " + "null argument" | "a count or a level is out of range" |
 *   "a modulus is even, below 3 or not below 2^61" | "a root word is not below its modulus" | "a scale is not finite and positive" |
 *   "a constant is not finite and below 2^63 in magnitude" | then, in chain order, "a scale ratio is not below 2^63" |
 *   "a constant times its scale is not finite". */
int lr_ckks_lincomb_constants(const uint64_t *moduli, const uint64_t *ntt_psi1, int n_moduli, double default_scale, int res_level,
                              double res_scale, int has_const, double c0_re, double c0_im, int n_terms, const double *term_re,
                              const double *term_im, const double *term_scale, const int *term_level, int *level_after,
                              double *scale_after, uint64_t *add_lo, uint64_t *add_hi, uint8_t *has_pre, uint64_t *pre, uint64_t *lo,
                              uint64_t *hi);
/* lr_ckks_lincomb: the element loops of the same chain as one device call.  Per limb i <= level, coefficient j and component u, with
 * s(j) = j < N/2 ? lo : hi:
 *     acc_u = accumulate ? out_u[i][j] : 0
 *     if add_lo:      acc_0 = CRed(acc_0 + add(j)[i])                         (component 0 only; AddConst :433, :441)
 *     for k in order: if has_pre[k]: acc_u = MRed(acc_u, pre[k][i])           (MultByConst :715, :728)
 *                     acc_u = CRed(acc_u + MRed(x_{k,u}[i][j], s_k(j)[i]))    (:591, :604)
 *     out_u[i][j] = acc_u
 * -- the same bits as lr_half_scalar_op with op 0, then per term op 1 and op 2, on a receiver zeroed when accumulate == 0, for every
 * input that sequence accepts (values need not be canonical).  One streaming pass per sixteen terms (T + 1 row passes per component
 * where the sequence moves 3 T to 5 T); more terms are chained through the receiver.  n_terms >= 0, no upper limit; n_terms == 0
 * with a constant is a valid call.  has_pre / pre / lo / hi: host arrays [n_terms] and [n_terms][level+1] (rows level+1 words apart:
 * lr_ckks_lincomb_constants' layout at level = level_after); add_lo / add_hi [level+1], or both NULL.  Every term and the receiver
 * carry the same batch (at most 32767); a term may appear twice; no term may share memory with a receiver poly; out_c0 != out_c1.
 * The constants travel in the launches' arguments: asynchronous on the context's stream, no host synchronisation, capturable.
 * Checks, in this order; a refused call writes nothing.  Messages "CKKS linear combination: " +
 *   LR_ERR_ARG          "null argument" | "n_terms is negative" | "a term is null" | "add_lo and add_hi come together or not at all" |
 *                       "the two components of the receiver share memory" | "a term shares memory with the receiver"
 *   LR_ERR_SHAPE        "level out of range" | "ring degree mismatch" | "a poly has fewer limbs than level + 1" |
 *                       "every term and the receiver carry the same batch" | "batch above 32767"
 *   LR_ERR_UNSUPPORTED  "ring degree below 4" */
int lr_ckks_lincomb(lr_context *ctxQ, int level, int n_terms, const lr_poly *const *terms_c0, const lr_poly *const *terms_c1,
                    const uint8_t *has_pre, const uint64_t *pre, const uint64_t *lo, const uint64_t *hi, const uint64_t *add_lo,
                    const uint64_t *add_hi, int accumulate, lr_poly *out_c0, lr_poly *out_c1);
/* ------------------------------------------------------------------ CKKS Add / Sub of any scale, level and degree */
/* evaluator.Add / AddNoMod / Sub / SubNoMod (ckks/evaluator.go:153-211) through evaluateInPlace (:227-342): the step between two products
 * of recurse / recurseCheby (MulRelin, Add(res, tmp, res), Rescale) and of computePowerBasisCheby (ckks/chebyshev_evaluation.go:86-99).
 * It is not a plain AddLvl: where the operands' scales differ the one of the smaller scale is first multiplied by uint64(ratio) with
 * MultByConst -- into the evaluator's pool ciphertext, or in place when that operand is the receiver --, the components that one operand
 * has beyond the other are copied, and Sub / SubNoMod negate them afterwards when they come from the subtrahend (:186-192, :203-209).
 * Split as the linear combination above: the scalar lines and the element loops.
 *
 * lr_ckks_combine_constants: the scalar lines of evaluateInPlace and the degree rules of its four callers, literally.  HOST ONLY: no
 * context, no device, thread-safe.
 *   in : moduli[n_moduli]; op = LR_ADD | LR_ADD_NOMOD | LR_SUB | LR_SUB_NOMOD; degree (0..2), level and scale of operand a (op0), of
 *        operand b (op1) and of the receiver before the call; receiver = which operand the receiver is (lr_ckks_combine_receiver; BOTH:
 *        a is b is the receiver, Add(C, C, C)).  A receiver that is an operand carries that operand's degree, level and scale.
 *   out: *level_after = the minimum of the three levels (:231); *scale_after = the larger scale (:328); *degree_after = the larger
 *        operand degree (Resize :237 -- a receiver of higher degree is cut down to it); *mult_side = 0 none, 1 a, 2 b: in each of the
 *        three branches :243-322 the operand of the SMALLER scale; mult[level_after+1] = per limb MForm(scaleUpExact(float64(r), 1, q_i))
 *        with r = uint64(larger / smaller) (:669-671, :698-709), written only when *mult_side != 0.
 *   The ratio is truncated: 1.5 multiplies by 1, and the multiplication still takes place (MRed by MForm(1) reduces the operand), as
 *   in the reference.  The uint64 reaches MultByConst's float64 (:670), so above 2^53 it is rounded before scaleUpExact sees it.
 *   Levels: the receiver is dropped by ctOut.Level() - min(a.Level, b.Level) (:238, DropLevel :901-914); one already at level 0 is left
 *   alone (the error return is ignored); the words are produced for the limbs 0..level_after, which is all that the element loops read.
 *   Where the reference panics the call returns LR_ERR_UNSUPPORTED: both operands of degree 0 (:117); a receiver whose degree is below
 *   the larger operand degree (:121); a receiver above level 0 and below both operand levels (the difference at :238 wraps and :910
 *   slices out of range); an operand to be multiplied that has degree 2 and is not the receiver (it would be written into the pool
 *   ciphertext of degree 1, :106, and MultByConst :711-716 indexes out of range).
 *   Domain, as for lr_ckks_lincomb_constants: finite positive scales, the ratio below 2^63, moduli odd and in [3, 2^61).  Outside it:
 *   LR_ERR_ARG.  Inside it the reference's guards `uint64(ratio) != 0` (:249, :255, :275, :281, :302, :312) cannot fail: x > y > 0 gives
 *   x / y >= 1.  A refused call writes NOTHING.
 *   Checked in this order, messages "CKKS combine constants: " +
 *   LR_ERR_ARG          "null argument" | "a count, the operation, the receiver, a degree or a level is out of range" |
 *                       "a modulus is even, below 3 or not below 2^61" | "a scale is not finite and positive" |
 *                       "the receiver is an operand and differs from it in degree, level or scale" | "a scale ratio is not below 2^63"
 *   LR_ERR_UNSUPPORTED  "both operands have degree 0" | "the receiver's degree is below the larger operand degree" |
 *                       "the receiver lies above level 0 and below both operand levels" |
 *                       "the operand to be multiplied has degree 2 and is not the receiver" */
typedef enum lr_ckks_combine_receiver {
    LR_COMBINE_OUT_NEW = 0,     /* neither operand                  the third branch, :296 */
    LR_COMBINE_OUT_A = 1,       /* ctOut == c0                      :243 */
    LR_COMBINE_OUT_B = 2,       /* ctOut == c1                      :270 */
    LR_COMBINE_OUT_BOTH = 3     /* ctOut == c0 == c1                :243 with equal scales */
} lr_ckks_combine_receiver;
int lr_ckks_combine_constants(const uint64_t *moduli, int n_moduli, int op, int a_degree, int a_level, double a_scale, int b_degree,
                              int b_level, double b_scale, int out_degree, int out_level, double out_scale, int receiver,
                              int *level_after, double *scale_after, int *degree_after, int *mult_side, uint64_t *mult);
/* lr_ckks_combine: the element loops as one device call.  Per limb i <= level, coefficient j and component u <= max(a_degree, b_degree),
 * with s(j) = j < N/2 ? lo : hi:
 *     x = a_u[i][j]               (u <= a_degree)            y = b_u[i][j]      (b given and u <= b_degree)
 *     if double_a:  x = CRed(x + x)                          Add(C, C, C) of computePowerBasisCheby, chebyshev_evaluation.go:92
 *     if ma:        x = MRed(x, ma(j)[i])                    MultByConst :715, :728
 *     if mb:        y = MRed(y, mb(j)[i])
 *     both present: r = CRed(x + y) | x + y | CRed((x + q) - y) | (x + q) - y              ring/ring.go:26, :48, :70, :94
 *     only x:       r = x                                    CopyLvl :335
 *     only y:       r = y for the two additions, q - y for the two subtractions            :339, NegLvl :190 / :207 (q - 0 stays q)
 *     if add and u == 0:  r = CRed(r + add(j)[i])            AddConst :433, :441
 *     out_u[i][j] = r
 * -- the same bits as today's sequence of lr_half_scalar_op (op 1, op 0) and lr_ewise (ADD.., NEG, COPY) calls on every input that
 * sequence accepts (values need not be canonical): all of evaluateInPlace with Sub's tail; the Chebyshev step 2 x - r y; 2 x + constant
 * (b NULL); the affine head m x + c of EvaluateCheby* (b NULL, ma_lo != ma_hi).  a: a_degree+1 polys; b: b_degree+1 polys, or NULL
 * (b_degree is then not read, and op only has to be valid); out: max(a_degree, b_degree)+1 polys.  ma / mb / add: (lo, hi) host arrays
 * of level+1 words each, or both NULL -- lr_ckks_combine_constants' mult for lo and hi alike; the words of AddConst and of a complex
 * MultByConst are the caller's, as for lr_half_scalar_op (lr_ckks_lincomb_constants with n_terms == 0 yields AddConst's).
 * Memory: out_u may be the very poly a_u or b_u (upstream's in-place case; every element is read before it is written); any other
 * overlap with the receiver is refused.  An operand poly may have batch 1 and is then read for every member; otherwise all batches are
 * equal, at most 32767 (21845 with three components: component and member share one grid axis).
 * The constants travel in the launch's arguments, every limb in one launch: asynchronous on the context's stream, no host
 * synchronisation, capturable.  Checks, in this order; a refused call writes nothing.  Messages "CKKS combine: " +
 *   LR_ERR_ARG          "null argument" | "no operand given" | "the operation is not LR_ADD, LR_ADD_NOMOD, LR_SUB or LR_SUB_NOMOD" |
 *                       "a degree is outside 0..2" | "a component is null" |
 *                       "the two words of a multiplier or of the constant come together or not at all" | "a multiplier of b without b" |
 *                       "the components of the receiver share memory" |
 *                       "an operand shares memory with the receiver other than component by component in place"
 *   LR_ERR_SHAPE        "level out of range" | "ring degree mismatch" | "a poly has fewer limbs than level + 1" |
 *                       "the receiver's components carry one batch, an operand that batch or 1" | "batch above 32767" |
 *                       "batch above 21845 at degree 2"
 *   LR_ERR_UNSUPPORTED  "ring degree below 4" */
int lr_ckks_combine(lr_context *ctxQ, int op, int level, int a_degree, const lr_poly *const *a, int b_degree, const lr_poly *const *b,
                    int double_a, const uint64_t *ma_lo, const uint64_t *ma_hi, const uint64_t *mb_lo, const uint64_t *mb_hi,
                    const uint64_t *add_lo, const uint64_t *add_hi, lr_poly *const *out);
/* ring.PermuteNTT (ring/ring_galois.go:55) on limbs 0..level: out[i][j] = in[i][index(j)], index(j) =
 * bitrev(((gen * (2*bitrev(j)+1) mod 2N) - 1) / 2), computed on the fly.  PermuteNTTWithIndex (:89) with the
 * table of PermuteNTTIndex(gen, power, N) (:29) is the same call with gen^power mod 2N.  Not in place
 * ("Careful, not inplace!"): in == out is LR_ERR_ARG. */
int lr_permute_ntt(lr_context *ctx, int level, const lr_poly *in, uint64_t gen, lr_poly *out);
/* PermuteNTTIndex (:29): host table of N entries */
int lr_permute_ntt_index(uint64_t gen, uint64_t power, uint64_t N, uint64_t *index);
/* Context.Permute (:106), coefficient domain, all limbs of the context: out[j][i*gen mod N] = +-in[j][i]
 * (a zero coefficient whose sign flips becomes q, as in the reference).  Not in place. */
int lr_permute(lr_context *ctx, const lr_poly *in, uint64_t gen, lr_poly *out);
/* Context.MultByMonomial (ring/ring.go:663): out = in * X^monomial_deg in Z_q[X]/(X^N+1), coefficient domain, all limbs.
 * Negated coefficients are q - x without reduction, as in the reference (a zero coefficient becomes q).  in == out is allowed
 * (staged through a temporary, as the reference's tmpx, :682). */
int lr_mult_by_monomial(lr_context *ctx, const lr_poly *in, uint64_t monomial_deg, lr_poly *out);

/* Context.Shift (ring/ring.go:575): out = in rotated left by n coefficient positions, every limb (n masked with (1 << N) - 1 as Go
 * evaluates it: all ones for N >= 64); n > N is the reference's slice panic: LR_ERR_ARG.  in == out is allowed. */
int lr_shift(lr_context *ctx, const lr_poly *in, uint64_t n, lr_poly *out);
/* Context.Rotate (ring/ring.go:775): coefficient j of every limb times omega^(n j), omega = psi^2, j = 1 .. N-1, canonical; coefficient 0
 * untouched.  The reference writes into p1 whatever its p2 argument is (:791), hence one poly here. */
int lr_rotate(lr_context *ctx, lr_poly *p1, uint64_t n);

/* ------------------------------------------------------------------ SimpleScaler --- */
/* NewSimpleScaler(t, context) (ring/ring_scaling.go:186): per modulus qi the integer part wi and the double-double
 * fractional part ti of ((Q/qi)^-1 mod qi) * t / qi, computed with the operation sequence of ring/float128.go.
 * t a power of two selects the masked reduction (:201-211), otherwise Montgomery / Barrett modulo t (:214-243).
 * t == 0 is LR_ERR_ARG (the reference divides by zero). */
int lr_simple_scaler_create(lr_context *ctx, uint64_t t, lr_simple_scaler **out);
int lr_simple_scaler_destroy(lr_simple_scaler *s);
/* host copies of wi[count] and ti[count][2] (hi, lo), count = number of moduli */
int lr_simple_scaler_tables(const lr_simple_scaler *s, uint64_t *wi, double *ti, int count);
/* SimpleScaler.Scale (:275): p2[j][i] = round(t/Q * p1[.][i]) mod t for every limb j of p2 (p2 may belong to another
 * context of the same degree, e.g. bfv's contextT; bfv/encoder.go:142).  p1 holds all moduli of the scaler's context,
 * coefficient domain.  p1 == p2 is allowed. */
int lr_simple_scale(lr_simple_scaler *s, const lr_poly *p1, lr_poly *p2);

/* ------------------------------------------------------------------ basis extension --- */
/* NewFastBasisExtender(contextQ, contextP), ring/ring_basis_extension.go:57 */
int lr_bext_create(lr_context *ctxQ, lr_context *ctxP, lr_bext **out);
int lr_bext_destroy(lr_bext *b);
/* ModUpSplitQP (:147): p1 over Q[0..level] -> p2 over all of P.  Coefficient domain. */
int lr_modup_split_qp(lr_bext *b, int level, const lr_poly *p1, lr_poly *p2);
/* ModUpSplitPQ (:154): p1 over P[0..level] -> p2 over all of Q. */
int lr_modup_split_pq(lr_bext *b, int level, const lr_poly *p1, lr_poly *p2);
/* ModDownNTTPQ (:163): p1 over Q||P (|Q|+|P| limbs, NTT domain; its P limbs are left in the
 * coefficient domain, as in Go) -> p2 over Q[0..level]. */
int lr_moddown_ntt_pq(lr_bext *b, int level, lr_poly *p1, lr_poly *p2);
/* ModDownSplitedNTTPQ (:207): (p1Q, p1P) NTT domain -> p2; p1P is left in the coefficient domain. */
int lr_moddown_split_ntt_pq(lr_bext *b, int level, const lr_poly *p1Q, lr_poly *p1P, lr_poly *p2);
/* ModDownPQ (:248): p1 over Q[0..level]||P, coefficient domain. */
int lr_moddown_pq(lr_bext *b, int level, const lr_poly *p1, lr_poly *p2);
/* ModDownSplitedPQ (:281) */
int lr_moddown_split_pq(lr_bext *b, int level, const lr_poly *p1Q, const lr_poly *p1P, lr_poly *p2);
/* ModDownSplitedQP (:314): divide by Q, result over P[0..levelP]. */
int lr_moddown_split_qp(lr_bext *b, int levelQ, int levelP, const lr_poly *p1Q, const lr_poly *p1P, lr_poly *p2);
/* tables for parity tests: 0 = modDownParamsPQ [|Q|], 1 = modDownParamsQP [|P|] (:39-53) */
int lr_bext_get_table(const lr_bext *b, int which, uint64_t *dst, size_t dst_count);

/* NewDecomposer(Q, P), :415 */
int lr_decomposer_create(lr_context *ctxQ, lr_context *ctxP, lr_decomposer **out);
int lr_decomposer_destroy(lr_decomposer *d);
/* Decompose (:476): p0 over Q (coefficient domain) -> p1 over Q[0..level]||P. */
int lr_decompose(lr_decomposer *d, int level, int crt_decomp_level, const lr_poly *p0, lr_poly *p1);
/* DecomposeAndSplit (:601): -> p1Q over Q[0..level], p1P over P. */
int lr_decompose_and_split(lr_decomposer *d, int level, int crt_decomp_level, const lr_poly *p0,
                           lr_poly *p1Q, lr_poly *p1P);

/* ------------------------------------------------------------------ RNS rescale ------- */
/* In place on p0 (limbs = level+1); on return p0 owns one limb less (see lr_poly_set_limbs).
 * DivFloorByLastModulusNTT (ring/ring_scaling.go:9), DivFloorByLastModulus (:37),
 * DivRoundByLastModulusNTT (:72), DivRoundByLastModulus (:117). */
int lr_div_floor_by_last_modulus_ntt(lr_context *ctx, lr_poly *p0);
int lr_div_floor_by_last_modulus(lr_context *ctx, lr_poly *p0);
int lr_div_round_by_last_modulus_ntt(lr_context *ctx, lr_poly *p0);
int lr_div_round_by_last_modulus(lr_context *ctx, lr_poly *p0);
/* ...Many / ...ManyNTT (:58,65,153,160) */
int lr_div_floor_by_last_modulus_many(lr_context *ctx, lr_poly *p0, int nb_rescales, int ntt_domain);
int lr_div_round_by_last_modulus_many(lr_context *ctx, lr_poly *p0, int nb_rescales, int ntt_domain);

/* ------------------------------------------------------------------ caller sequences -- */
/* The ring-level call sequence of ckks.Evaluator, kept on the device for a whole batch.
 * lr_ckks_plan owns what ckks.NewEvaluator builds: FastBasisExtender, Decomposer and the
 * scratch pools (ckks/evaluator.go:81-112). */
int lr_ckks_plan_create(lr_context *ctxQ, lr_context *ctxP, int max_batch, lr_ckks_plan **out);
/* the same with explicit options; NULL = the options of ctxQ (what lr_ckks_plan_create does) */
int lr_ckks_plan_create_ex(lr_context *ctxQ, lr_context *ctxP, int max_batch, const lr_options *opt, lr_ckks_plan **out);
/* Diagnostics of the small-batch paths of the key switch (no reference counterpart).  forks: how often two independent launches of a
 * pipeline (the digits' P rows beside their Q rows; ModDown's two components) went out side by side on the plan's auxiliary stream
 * instead of in order -- done at N = 2^16 (where one workgroup of such a launch runs long enough to pay for the hand-over) while the
 * forked launch is far from filling the chip AND the plan is the only one alive on its device that is not a batcher's lane (a lone
 * evaluator); LR_NO_FORK=1 at plan creation switches it off.  grouped_extensions:
 * launches that carried the basis extensions of all digits of a key switch at once (LR_NO_EXT_GROUP=1: one launch per digit).
 * Results are the same bits either way.  Either pointer may be NULL. */
int lr_ckks_plan_stats(const lr_ckks_plan *plan, uint64_t *forks, uint64_t *grouped_extensions);
int lr_ckks_plan_destroy(lr_ckks_plan *plan);
/* switchKeysInPlace (ckks/evaluator.go:1475): cx over Q[0..level], NTT domain;
 * evk = SwitchingKey.evakey as one poly, batch = beta*2, limbs = |Q|+|P|
 * (ckks/keygen.go:68-70: evakey[i][0], evakey[i][1] in NTT + Montgomery form);
 * p0, p1 over Q[0..level] receive the two key-switched components (any strides; neither may alias cx). */
int lr_ckks_switch_keys(lr_ckks_plan *plan, int level, const lr_poly *cx, const lr_poly *evk,
                        lr_poly *p0, lr_poly *p1);
/* bfv.evaluator.switchKeys (bfv/evaluator.go:736-812) on the same plan (what bfv.NewEvaluator builds for it -- decomposer,
 * baseconverterQ1P, key-switch pools, bfv/evaluator.go:100-112 -- is what the CKKS plan holds): cx over all of Q in the
 * COEFFICIENT domain, evk = SwitchingKey.evakey as for lr_ckks_switch_keys (bfv/keygen.go: NTT + Montgomery form over Q||P);
 * p0, p1 <- the two key-switched polys over Q, coefficient domain.  cx, p0 and p1 must be distinct polys. */
int lr_bfv_switch_keys(lr_ckks_plan *plan, const lr_poly *cx, const lr_poly *evk, lr_poly *p0, lr_poly *p1);
/* bfv.evaluator.Relinearize of a degree-2 ciphertext (bfv/evaluator.go:480-501, 512-524): (out0, out1) = (c0 + p0, c1 + p1) with
 * (p0, p1) = switchKeys(c2, evakey.evakey[0]); every poly over Q, coefficient domain; out0 / out1 may be c0 / c1. */
int lr_bfv_relinearize(lr_ckks_plan *plan, const lr_poly *c0, const lr_poly *c1, const lr_poly *c2, const lr_poly *evk,
                       lr_poly *out0, lr_poly *out1);
/* bfv.evaluator.Relinearize for every degree (bfv/evaluator.go:480-499, 509-522) as ONE call:
 *   (a0, a1) = (ct[0], ct[1]);  for deg = degree .. 2:  (p0, p1) = switchKeys(ct[deg], evks[deg - 2]);
 *   a0 = CRed(a0 + p0); a1 = CRed(a1 + p1);   (out0, out1) <- (a0, a1)
 * bit for bit the reference's loop.  ct[0 .. degree] over all of Q, coefficient domain, one batch up to the plan's max_batch; evks[k] =
 * the image of evakey.evakey[k], the key that switches from s^(k + 2), in the layout lr_ckks_switch_keys reads (what
 * lr_keygen_relin_keys with n_powers = maxDegree, lr_setup_rkg_key and NewSwitchingKey().set produce).  1 <= degree <= 5, the reach of
 * lr_bfv_mul_deg; degree 1 copies (evks may then be NULL); degree 2 gives the bits of lr_bfv_relinearize.  The additions keep the
 * reference's order, the highest degree first, each with one conditional subtraction: the result is the composed sequence's for any
 * input lr_ewise ADD accepts, not only canonical ones.  out0 may be ct[0] and out1 may be ct[1]; an input that is not an output is left
 * unchanged.
 * Checks, in this order: LR_ERR_ARG for a null argument, a null entry of ct or, for degree >= 2, a null evks or a null entry of evks, a
 * degree outside 1 .. 5, out0 and out1 the same poly, an output that is ct[k] for k >= 2, out0 being ct[1] or out1 being ct[0] ("the
 * same poly": the same device rows); then LR_ERR_SHAPE for a batch beyond max_batch, a poly with fewer limbs than Q, of another ring
 * degree or another batch, a key image with a batch below 2 beta or fewer than |Q| + |P| limbs.  Nothing is written by a refused call.
 * Routes: the degree - 1 key switches share no data, so G = min(degree - 1, max(1, max_batch / batch)) of them, the
 * highest degrees first, run as ONE key switch over G * batch members with one key per group, and one pass adds their G results to the
 * running pair (the plan's scratch stays what a call at max_batch needs); plans or contexts with lr_options::no_epilogue run the
 * reference's sequence call by call: per degree the key switch and the two Adds of lr_bfv_relinearize.  Same bits on every route. */
int lr_bfv_relinearize_deg(lr_ckks_plan *plan, const lr_poly *const *ct, int degree, const lr_poly *const *evks, lr_poly *out0,
                           lr_poly *out1);
/* bfv.evaluator.permute (bfv/evaluator.go:711-735) = RotateRows (:670) with gen = galElRotRow, RotateColumns (:579) with the key of
 * that rotation and gen = galElRotColLeft[k], and one step of rotateColumnsPow2 (:636): Context.Permute of both components by the
 * Galois element `gen` (coefficient domain), switchKeys of the second with `rotkey`, Add + Copy.  Every poly over Q, coefficient
 * domain; (out_c0, out_c1) may be (c0, c1); out_c0 != out_c1. */
int lr_bfv_rotate(lr_ckks_plan *plan, const lr_poly *c0, const lr_poly *c1, uint64_t gen, const lr_poly *rotkey,
                  lr_poly *out_c0, lr_poly *out_c1);
/* A chain of bfv.evaluator.permute steps as ONE call (rotateColumnsPow2, bfv/evaluator.go:637-666, and the loop of InnerSum, :701-707).
 * The state (a0, a1) starts as (c0, c1); step i = 0 .. n_steps - 1, with Galois element gens[i] and key image keys[i], is permute
 * (:711-733): (e0, e1) = Permute of both components by gens[i]; (p0, p1) = switchKeys(e1, keys[i]); (r0, r1) = (CRed(e0 + p0), p1); then
 *   accumulate == 0:  (a0, a1) <- (r0, r1)                               rotateColumnsPow2 :653-665 (gens: the generator's squarings at the
 *                                                                        set bits of k, keys: evakeyRotCol[2^i] of those bits)
 *   accumulate != 0:  (a0, a1) <- (CRed(r0 + a0), CRed(r1 + a1))         InnerSum :702-703, :706-707
 * and (out_c0, out_c1) <- the last state; bit for bit the reference's call sequence.  Every poly over all of Q, coefficient domain,
 * inputs in [0, q); any batch up to the plan's max_batch; (out_c0, out_c1) may be (c0, c1), an input that is not an output is left
 * unchanged; one key handle may serve several steps; n_steps == 0 copies (gens and keys may then be NULL).
 * Checks, in this order: LR_ERR_ARG for a null argument or a null entry of keys, n_steps < 0, an even Galois element, out_c0 and out_c1
 * the same poly; then LR_ERR_SHAPE for a batch beyond max_batch, a poly with fewer limbs than Q, of another degree or another batch.
 * Nothing is written by a refused call.  Each step is the key switch plus one fused pass where a coefficient row fits
 * the LDS (2^11 <= N <= 2^14); other degrees, plans or contexts with lr_options::no_epilogue, and the replacing chain of a single
 * ciphertext at N = 2^14 (measured) run the step from the separate Permute / Add launches.  Same bits on every route.
 * The plan keeps four more polys over Q per batch member for its chains. */
int lr_bfv_rotate_chain(lr_ckks_plan *plan, const lr_poly *c0, const lr_poly *c1, int n_steps, const uint64_t *gens,
                        const lr_poly *const *keys, int accumulate, lr_poly *out_c0, lr_poly *out_c1);
/* bfv.evaluator.InnerSum (bfv/evaluator.go:691-708): the accumulating chain over galElRotColLeft[2^i] = 5^(2^i) mod 2N with
 * col_keys[i] = the image of evakeyRotColLeft[2^i], i = 0 .. log2(N) - 2, and then galElRotRow = 2N - 1 with row_key; the Galois
 * elements are computed here.  N = 2 has no column step (n_col_keys == 0, col_keys may be NULL).  Polys, batch, aliasing and routes as
 * for lr_bfv_rotate_chain.  Checks, in this order: LR_ERR_ARG for a null argument or a null entry of col_keys, out_c0 and out_c1 the
 * same poly, n_col_keys != log2(N) - 1; then the LR_ERR_SHAPE checks of lr_bfv_rotate_chain. */
int lr_bfv_inner_sum(lr_ckks_plan *plan, const lr_poly *c0, const lr_poly *c1, int n_col_keys, const lr_poly *const *col_keys,
                     const lr_poly *row_key, lr_poly *out_c0, lr_poly *out_c1);
/* MulRelin (ckks/evaluator.go:1016), ciphertext x ciphertext, with evaluation key.
 * ct0_c0/ct0_c1 etc. are the degree-0/1 components (Ciphertext.Value()[0], [1]). */
int lr_ckks_mulrelin(lr_ckks_plan *plan, int level, const lr_poly *ct0_c0, const lr_poly *ct0_c1,
                     const lr_poly *ct1_c0, const lr_poly *ct1_c1, const lr_poly *evk,
                     lr_poly *out_c0, lr_poly *out_c1);
/* Batcher for the reference's concurrency model -- one evaluator per goroutine, one ciphertext per call
 * (examples/dbfv/psi/psi.go:215-233, examples/ckks: each worker holds its own ckks.Evaluator).  Concurrent calls of
 * lr_ckks_batcher_mulrelin from any number of host threads are merged into batched launches: a call queues its request, and whichever
 * caller finds a free lane runs everything queued with the same (level, evk) -- up to max_batch polys, in arrival order -- as ONE
 * MulRelin (the operands are read in place through a pointer table, the results are copied out to the callers' polys by one kernel),
 * waits for it and wakes the others.  The call returns when its own result is complete on the device (it may be used on any
 * stream afterwards); operands are synchronised with the streams of the contexts they were created on before they are queued.
 * plans[i]: one plan per lane, each over its OWN pair of contexts, same moduli, device and max_batch; the batcher creates one
 * stream per lane and sets it on the lane's contexts (lr_context_set_stream; destroy puts the library's stream back).  The lanes'
 * streams are created in different priority classes (lane 0 the device's greatest priority, lane 1 its least, lane 2 the default,
 * ...): the runtime binds a stream to a hardware queue of its class, and two lanes on one queue would run one after the other.  Two lanes
 * let the next batch's launches overlap the running one.  The plans and contexts stay owned by the caller and must outlive the
 * batcher; while it exists they are not used for anything else.  evk must be the SAME key image handle in the calls that are to
 * share a batch (the relinearisation key is shared by the evaluators of one party, ckks/evaluator.go:1016).
 * Results are the same bits as lr_ckks_mulrelin's.  An error of a batch is returned by every call that was part of it. */
typedef struct lr_ckks_batcher lr_ckks_batcher;
int lr_ckks_batcher_create(lr_ckks_plan *const *plans, int n_lanes, lr_ckks_batcher **out);
void lr_ckks_batcher_destroy(lr_ckks_batcher *batcher);
int lr_ckks_batcher_mulrelin(lr_ckks_batcher *batcher, int level, const lr_poly *ct0_c0, const lr_poly *ct0_c1,
                             const lr_poly *ct1_c0, const lr_poly *ct1_c1, const lr_poly *evk, lr_poly *out_c0, lr_poly *out_c1);
/* The same for evaluator.permuteNTT (RotateColumns with the key of that rotation, Conjugate; ckks/evaluator.go:1448): calls with the
 * same (level, Galois element, key image) in flight together run as one batched lr_ckks_rotate.  Same bits as lr_ckks_rotate; the
 * outputs may be the inputs.  MulRelin and rotation requests never share a launch; they take the lanes in arrival order. */
int lr_ckks_batcher_rotate(lr_ckks_batcher *batcher, int level, const lr_poly *ct_c0, const lr_poly *ct_c1, uint64_t galois_element,
                           const lr_poly *rotkey, lr_poly *out_c0, lr_poly *out_c1);
/* launches so far, polys they carried, the largest batch (any of the pointers may be NULL) */
int lr_ckks_batcher_stats(lr_ckks_batcher *batcher, uint64_t *batches, uint64_t *products, int *largest);
/* MulRelin with evakey == nil (ckks/evaluator.go:1038-1111): the degree-2 result (out_c0, out_c1, out_c2), no key switch.
 * Outputs may alias the inputs (ctOut == ct0 / ct1: the reference goes through its pools and copies, :1105-1111); ct0 == ct1 is
 * the squaring branch (:1083-1088), whose result equals the regular branch's on the same operands. */
int lr_ckks_mul_norelin(lr_ckks_plan *plan, int level, const lr_poly *ct0_c0, const lr_poly *ct0_c1,
                        const lr_poly *ct1_c0, const lr_poly *ct1_c1, lr_poly *out_c0, lr_poly *out_c1, lr_poly *out_c2);
/* MulRelin, plaintext x ciphertext branch (ckks/evaluator.go:1113-1131): out_ck = MRed(MForm(pt), ct_ck).  pt: the plaintext's
 * value (NTT domain), batch 1 (broadcast) or the ciphertexts' batch. */
int lr_ckks_mul_plain(lr_ckks_plan *plan, int level, const lr_poly *pt, const lr_poly *ct_c0, const lr_poly *ct_c1,
                      lr_poly *out_c0, lr_poly *out_c1);
/* pkEncryptor.encrypt, the branch through the special primes, after the sampling (ckks/encryptor.go:205-234):
 * ct = ModDownPQ(InvNTT(u * pk_k) + e_k) -> NTT, + pt on component 0.  u (SampleTernaryMontgomeryNTT, :206), pk0 / pk1 and
 * e0 / e1 (the residues gaussianSampler.SampleAndAdd adds, coefficient domain, values in [0, q]) hold |Q|+|P| limbs in contextQP's
 * order; pk may have batch 1.  pt over Q[0..level], NTT domain.  Sampling stays on the host (out of scope).
 * The reference's Context.NTT at :229 walks every modulus of contextQ (a Go index panic for level < |Q|-1); here limbs 0..level. */
int lr_ckks_encrypt_pk(lr_ckks_plan *plan, int level, const lr_poly *u, const lr_poly *pk0, const lr_poly *pk1,
                       const lr_poly *e0, const lr_poly *e1, const lr_poly *pt, lr_poly *out_c0, lr_poly *out_c1);
/* decryptor.Decrypt (ckks/decryptor.go:53-78): Horner evaluation of ct[0..degree] at the secret key (NTT + Montgomery form,
 * batch 1 or the ciphertexts' batch) with the reference's lazy-reduction cadence; pt_out over Q[0..level]. */
int lr_ckks_decrypt(lr_ckks_plan *plan, int level, const lr_poly *const *ct, int degree, const lr_poly *sk, lr_poly *pt_out);
/* Rescale, one level (ckks/evaluator.go:933-968 inner loop): DivRoundByLastModulusNTT on both components. */
int lr_ckks_rescale(lr_ckks_plan *plan, lr_poly *c0, lr_poly *c1);
/* permuteNTT (ckks/evaluator.go:1448-1468), the body of RotateColumns with a specific rotation key (:1222) and of
 * Conjugate (:1446): both components are permuted by the Galois element `gen` (what ring.PermuteNTTIndex turns
 * into RotationKeys.permuteNTTLeftIndex[k] / permuteNTTConjugateIndex), the second is key-switched with `rotkey`
 * (a SwitchingKey image as for lr_ckks_switch_keys).  out may alias the input. */
int lr_ckks_rotate(lr_ckks_plan *plan, int level, const lr_poly *c0, const lr_poly *c1, uint64_t gen,
                   const lr_poly *rotkey, lr_poly *out_c0, lr_poly *out_c1);
/* A chain of evaluator.permuteNTT steps as ONE call (rotateColumnsPow2, ckks/evaluator.go:1402-1424 -- the path of every RotateColumns
 * when only the power-of-two keys of GenRotationKeysPow2 exist -- and the slot-sum loop RotateColumns(ct, 2^i, tmp); Add(ct, tmp, ct)).
 * The state (a0, a1) starts as (c0, c1) over Q[0..level], NTT domain; step i = 0 .. n_steps - 1, with Galois element gens[i] and key
 * image keys[i], is permuteNTT (:1452-1471): (e0, e1) = PermuteNTT of both components by gens[i] (:1458-1459);
 * (p0, p1) = switchKeysInPlace(level, e1, keys[i]) (:1464); (r0, r1) = (CRed(e0 + p0), p1) (:1466-1467); then
 *   accumulate == 0:  (a0, a1) <- (r0, r1)                               rotateColumnsPow2 :1414-1423 (gens: the Galois elements of the
 *                                                                        rotations by 2^i at the set bits of k, keys: their keys)
 *   accumulate != 0:  (a0, a1) <- (CRed(r0 + a0), CRed(r1 + a1))         RotateColumns into a temporary, then Add at equal scales
 * and (out_c0, out_c1) <- the last state; bit for bit the composed sequence for inputs in [0, q).  Any batch up to the plan's
 * max_batch; (out_c0, out_c1) may be (c0, c1) or (c1, c0), an input that is not an output is left unchanged; one key handle may serve
 * several steps; n_steps == 0 copies (gens and keys may then be NULL).  The polys need not share a stride.
 * Checks, in this order: LR_ERR_ARG for a null argument or a null entry of keys, n_steps < 0, an even Galois element, out_c0 and out_c1
 * the same poly; then LR_ERR_SHAPE for a level out of range, a batch beyond max_batch, a poly with fewer limbs than level + 1, of
 * another degree or another batch, a key image with fewer than 2 * beta polys or |Q| + |P| limbs.  Nothing is written by a refused call.
 * An accumulating step is one pass in front of the key switch (its input and the first component's addend, the running sum already in
 * it) and the key switch, whose last pass adds the running second component: no Add is launched.  Plans or contexts with
 * lr_options::no_epilogue, and rings whose forward transform has no epilogue, run the step as lr_ckks_rotate does and the two Adds
 * after it.  A replacing step has no Add to lose and is lr_ckks_rotate's launches on every plan (measured), written
 * straight into the outputs.  Same bits on every route.  An accumulating chain keeps four more polys over Q[0..level] per batch member
 * in the plan. */
int lr_ckks_rotate_chain(lr_ckks_plan *plan, int level, const lr_poly *c0, const lr_poly *c1, int n_steps, const uint64_t *gens,
                         const lr_poly *const *keys, int accumulate, lr_poly *out_c0, lr_poly *out_c1);
/* ------------------------------------------------------------------ CKKS power basis (monomial and Chebyshev) */
/* The products of EvaluatePoly* / EvaluateCheby*: computePowerBasis (ckks/polynomial_evaluation.go:76-93), C[n] = C[a] C[b], and
 * computePowerBasisCheby (ckks/chebyshev_evaluation.go:60-101), C[n] = 2 C[a] C[b] - C[c], with a = ceil(n / 2), b = n >> 1, c = a - b
 * and C[0] the constant 1; each product is MulRelinNew, Rescale(., ckksContext.scale, .) and, Chebyshev, Add(C[n], C[n], C[n]) followed
 * by AddConst(C[n], -1, C[n]) (c == 0) or Sub(C[n], C[c], C[n]).  PowerOf2 (ckks/algorithms.go:9-31) is computePowerBasis(2^k).  Split as
 * the calls above: the scalar lines and the element loops.  The recurse / recurseCheby drivers stay with the caller.
 *
 * lr_ckks_power_basis_schedule: the scalar lines, literally.  HOST ONLY: no context, no device, thread-safe.
 *   in : moduli[n_moduli]; default_scale = ckksContext.scale, Rescale's threshold; chebyshev != 0: computePowerBasisCheby; level and scale
 *        of C[1]; targets[n_targets], each in 1 .. 65535: the n of the caller's computePowerBasis(n) calls, in its order; capacity = the
 *        products that `products` holds and the rows that mult and add hold, n_moduli words each.
 *   out: *n_products; products[k], k < *n_products, in the order the reference creates them: for each target the recursion of :78-92 /
 *        :70-99 -- first a, then b, each only when not yet present (c is 0 or 1 and C[1] is always present, so c never recurses); a
 *        target that is 1 or already present adds nothing.  Per product (lr_ckks_basis_product): scale = s_a s_b (:1038) at
 *        mul_level = min of the operands' levels (:1005); Rescale's loop `scale >= threshold * float64(q_level) / 2 && level != 0`
 *        (:945-961; at level 0 nothing, the error return is ignored by the caller) divides the scale by float64(q_level) n_rescales
 *        times; tail 1 is lr_ckks_combine_constants(LR_SUB, a = C[n] after Add(C, C, C), b = C[1], receiver = a): mult_side, the mult
 *        row, the larger scale, the level; tail 2 leaves level and scale and its add row is scaleUpExact(-1, scale, q_i) for
 *        i <= level_after, one word per limb for both halves of the row (the constant is real).  Rows and words that are not used are 0.
 *   Domain, as for lr_ckks_lincomb_constants and lr_ckks_combine_constants: finite positive scales (every product's included), a scale
 *   ratio below 2^63, moduli odd and in [3, 2^61).  A refused call writes NOTHING, with one exception: "more products than capacity"
 *   sets *n_products to the number needed, so a caller sizes its buffers with capacity == 0 (products, mult and add may then be NULL)
 *   and calls again.  Every refusal is LR_ERR_ARG; checked in this order, messages "CKKS power basis schedule: " +
 *     "null argument" | "a count or a level is out of range" | "a target is 0 or above 65535" |
 *     "a modulus is even, below 3 or not below 2^61" | "a scale is not finite and positive" (default_scale, c1_scale) |
 *     "more products than capacity" | then per product, in order: "a scale is not finite and positive" (s_a s_b) |
 *     "a scale ratio is not below 2^63" (tail 1).
 *   Example of the last: PN12QP109, Chebyshev, targets beyond 2 -- the products stall at level 0, their scales square, and the ratio
 *   to C[1] leaves the domain; the monomial form of the same call is accepted with n_rescales == 0. */
typedef struct lr_ckks_basis_product {
    uint32_t n, a, b, c;     /* C[n] = C[a] C[b]; a = ceil(n/2), b = n >> 1; Chebyshev: c = a - b (0: the constant 1, else 1); monomial: 0 */
    int32_t  mul_level;      /* min(level of C[a], level of C[b]): MulRelinNew :1005, MulRelin :1020 */
    int32_t  n_rescales;     /* iterations of Rescale's loop :945-961; 0 at level 0 or below the threshold */
    int32_t  level_after;
    int32_t  layer;          /* 1 + the largest layer among C[a], C[b]; C[1] is layer 0 */
    int32_t  tail;           /* 0 none (monomial) | 1: 2 x - C[c] (Add :92, Sub :98) | 2: 2 x + const (Add :92, AddConst(-1) :96) */
    int32_t  mult_side;      /* tail 1: lr_ckks_combine_constants' mult_side for Sub(C[n], C[c], C[n]), receiver = a; else 0 */
    double   scale_after;
} lr_ckks_basis_product;
int lr_ckks_power_basis_schedule(const uint64_t *moduli, int n_moduli, double default_scale, int chebyshev, int c1_level, double c1_scale,
                                 int n_targets, const uint32_t *targets, int capacity, int *n_products, lr_ckks_basis_product *products,
                                 uint64_t *mult, uint64_t *add);      /* mult, add: [capacity][n_moduli] */
/* lr_ckks_power_basis: the element loops of a schedule as ONE device call.  Every C is a batch of c1_c0->batch ciphertexts of degree 1 in
 * the NTT domain; C[1] = (c1_c0, c1_c1) at c1_level; (outs_c0[k], outs_c1[k]) receives C[products[k].n] on limbs 0 .. level_after and
 * needs level_after + 1 limbs -- its logical limb count is left alone, the limbs above level_after are not written.  mult and add are
 * the schedule's rows, row_words words apart.  evk: the relinearisation key's image as for lr_ckks_mulrelin.  Bit for bit the composed
 * sequence per product -- lr_ckks_mulrelin at mul_level, n_rescales times lr_ckks_rescale, then the lr_ckks_combine call of the tail
 * (double_a with LR_SUB against C[1] and the mult row on mult_side, or with the add row) -- for inputs in [0, q).  The inputs are left
 * unchanged.  Any batch up to the plan's max_batch.
 * Merged route (default, where the forward transform has the epilogue): the products are grouped by (layer, mul_level, n_rescales) and
 * a group is cut into chunks of max(1, max_batch / batch) products; per chunk ONE MulRelin over products * batch members, whose
 * operands are read in place through a pointer table, into a staging pair of the plan; n_rescales one-level divisions of that pair (the
 * reference's loop, not the Many form); ONE tail pass that writes every C[n] to its polys.  The pointer tables and the
 * products' words travel in a small device table of the plan, filled by an asynchronous copy from eight pinned slots that an event
 * guards: the call is asynchronous on the contexts' stream (the device images are reused in stream order from call to call, which
 * lr_context_set_stream preserves when it replaces a stream).  It waits on the host in three
 * bounded cases: a slot handed out again while its copy is pending waits for that copy and so for the kernels queued before it (more
 * than eight chunks in flight); a slot, the staging pair or a pool of the plan that grows synchronises the stream, as the plan's other
 * calls do.  Not capturable.  A chunk of one product has nothing to merge and runs as the product stands.  Plans or contexts with lr_options::no_epilogue,
 * rings whose forward transform has no epilogue, batches above 32767 and the one shape measured level with the sequence (the widest
 * chunk a pair, 8 ciphertexts or more, N <= 2^15) run product by product from the existing calls: MulRelin, the
 * divisions and the lr_ckks_combine call of the tail -- a product that is divided goes through the plan's staging pair and its tail
 * writes the output, because the output holds level_after + 1 limbs only and nothing above them is written.  Same bits on every route.
 * The plan keeps the staging pair: two polys over Q[0..mul_level] per member of the largest chunk.
 * Checks, in this order; a refused call writes nothing.  Messages "CKKS power basis: " + (the shared checks of the plan's calls without it)
 *   LR_ERR_ARG          "null argument" (plan, C[1], evk) | "negative product count" | "null argument" (products, mult, add, outs) |
 *                       "an output is null" | "row_words is below c1_level + 1" | "the schedule is not self-consistent": per product,
 *                       an operand that is neither 1 nor an earlier product of a lower layer, n below 2 or listed before, mul_level
 *                       not the minimum of its operands' level_after (C[1]: c1_level), a tail or mult_side outside 0..2, n_rescales
 *                       outside 0..mul_level, level_after != mul_level - n_rescales, tail 1 with c != 1 |
 *                       "two outputs share memory" | "an output shares memory with C[1]"
 *   LR_ERR_SHAPE        "batch exceeds the plan's max_batch" | "level out of range" | "ring degree mismatch" |
 *                       "poly has fewer limbs than level+1" | "batch mismatch" (C[1] at c1_level, then each output at its level_after) |
 *                       "the two polys of an output must share their stride" | "evaluation key: need batch >= 2*beta and |Q|+|P| limbs"
 *   LR_ERR_UNSUPPORTED  "ring degree below 4"
 *   LR_ERR_ARG          the two contexts on different streams */
int lr_ckks_power_basis(lr_ckks_plan *plan, int n_products, const lr_ckks_basis_product *products, const uint64_t *mult,
                        const uint64_t *add, int row_words, int c1_level, const lr_poly *c1_c0, const lr_poly *c1_c1, const lr_poly *evk,
                        lr_poly *const *outs_c0, lr_poly *const *outs_c1);
/* RotateHoisted + switchKeyHoisted (ckks/evaluator.go:1252-1391): n_rot rotations of one ciphertext share the
 * digit decomposition of its second component.  gens[r], rotkeys[r] -> (outs_c0[r], outs_c1[r]); not in place. */
int lr_ckks_rotate_hoisted(lr_ckks_plan *plan, int level, const lr_poly *c0, const lr_poly *c1, int n_rot,
                           const uint64_t *gens, const lr_poly *const *rotkeys, lr_poly *const *outs_c0,
                           lr_poly *const *outs_c1);

/* bfv.Evaluator.Mul = tensorAndRescale (bfv/evaluator.go:467,278) for two degree-1 ciphertexts, device-resident
 * for a whole batch.  lr_bfv_plan owns what bfv.NewEvaluator builds for it: baseconverterQ1Q2 =
 * NewFastBasisExtender(contextQ, contextQMul), pHalf = (prod QMul) >> 1 and the scratch pools (bfv/evaluator.go:89-112). */
typedef struct lr_bfv_plan lr_bfv_plan;
int lr_bfv_plan_create(lr_context *ctxQ, lr_context *ctxQMul, uint64_t t, int max_batch, lr_bfv_plan **out);
/* the same with explicit options; NULL = the options of ctxQ */
int lr_bfv_plan_create_ex(lr_context *ctxQ, lr_context *ctxQMul, uint64_t t, int max_batch, const lr_options *opt, lr_bfv_plan **out);
int lr_bfv_plan_destroy(lr_bfv_plan *plan);
/* operands and results over Q in the coefficient domain, as BFV ciphertexts are; out has degree 2.  ct0 == ct1 (the same two handles: the
 * reference's squaring case, bfv/evaluator.go:306,334-349) lifts and transforms the operand once; outputs may be operands. */
int lr_bfv_mul(lr_bfv_plan *plan, const lr_poly *ct0_c0, const lr_poly *ct0_c1, const lr_poly *ct1_c0,
               const lr_poly *ct1_c1, lr_poly *out_c0, lr_poly *out_c1, lr_poly *out_c2);
/* bfv.Evaluator.Mul for every operand degree: tensorAndRescale's branch for operands that are not both of degree 1
 * (bfv/evaluator.go:371-415), e.g. a ciphertext times a Plaintext (an element of degree 0) or a product with an unrelinearised
 * degree-2 result.  ct0[0..deg0], ct1[0..deg1] and out[0..deg0+deg1] over Q in the coefficient domain, one batch, batch <= max_batch.
 * deg0, deg1 >= 0 and 1 <= deg0 + deg1 <= 5 (bfv.NewEvaluator's pools hold 6 polys, :74-82), else LR_ERR_ARG; shapes as lr_bfv_mul.
 * deg0 == deg1 with ct1[i] == ct0[i] for every i (the same handles: Go's el0 == el1) is the squaring case (:379-402): the operand
 * is lifted and transformed once.  (1, 1) is lr_bfv_mul.  Every operand is lifted before any output is written, so an output may
 * be an operand; the outputs must be distinct handles (LR_ERR_ARG). */
int lr_bfv_mul_deg(lr_bfv_plan *plan, const lr_poly *const *ct0, int deg0, const lr_poly *const *ct1, int deg1,
                   lr_poly *const *out);

/* The batcher for the workload the reference itself pools: every task of examples/dbfv/psi/psi.go:215-233 runs evaluator.Mul and
 * evaluator.Relinearize on one BFV ciphertext pair.  Concurrent calls from any number of host threads are merged into batched launches
 * as by lr_ckks_batcher: a call queues its request, whichever caller finds a free lane runs everything queued of the same kind (and, for
 * Relinearize, the same key image handle) -- up to max_batch polys, in arrival order -- and wakes the others; the call returns when its own
 * result is complete on the device.  The callers' polys are read and written in place through a pointer table (one gather and one
 * scatter kernel around the staged pipeline).  mul_plans[i] / ks_plans[i]: one lr_bfv_plan over (contextQ_i, contextQMul_i) and one
 * lr_ckks_plan over the SAME contextQ_i and (contextQ_i, contextP_i) per lane -- the two halves of what bfv.NewEvaluator builds
 * (bfv/evaluator.go:89-112) -- each lane over its own contexts, same moduli, device, t and max_batch; ks_plans may be NULL (no
 * Relinearize).  The batcher sets one stream per lane on the lane's contexts; plans and contexts stay owned by the caller, must outlive
 * the batcher and are used for nothing else while it exists (destroying one first is LR_ERR_ARG).  Same bits as lr_bfv_mul /
 * lr_bfv_relinearize; an error of a batch is returned by every call that was part of it. */
typedef struct lr_bfv_batcher lr_bfv_batcher;
int lr_bfv_batcher_create(lr_bfv_plan *const *mul_plans, lr_ckks_plan *const *ks_plans, int n_lanes, lr_bfv_batcher **out);
void lr_bfv_batcher_destroy(lr_bfv_batcher *batcher);
/* evaluator.Mul (bfv/evaluator.go:467) of two degree-1 ciphertexts: coefficient domain, degree-2 result */
int lr_bfv_batcher_mul(lr_bfv_batcher *batcher, const lr_poly *ct0_c0, const lr_poly *ct0_c1, const lr_poly *ct1_c0, const lr_poly *ct1_c1,
                       lr_poly *out_c0, lr_poly *out_c1, lr_poly *out_c2);
/* evaluator.Relinearize (bfv/evaluator.go:512) of a degree-2 ciphertext with the key image evk (one handle for all callers) */
int lr_bfv_batcher_relinearize(lr_bfv_batcher *batcher, const lr_poly *c0, const lr_poly *c1, const lr_poly *c2, const lr_poly *evk,
                               lr_poly *out0, lr_poly *out1);
int lr_bfv_batcher_stats(lr_bfv_batcher *batcher, uint64_t *batches, uint64_t *products, int *largest);

/* bfv.Encoder (bfv/encoder.go:10-182) for a batch of plaintexts, device-resident.  lr_bfv_encoder owns what bfv.NewEncoder builds (:28-68):
 * contextT = (N, [t]) with the reference's psi, indexMatrix (:36-58, GaloisGen = 5), deltaMont = GenLiftParams(contextQ, t)
 * (bfv/utils.go:9-23), NewSimpleScaler(t, contextQ) and the one-limb polypool, for up to max_batch plaintexts per call.  A t that does not
 * allow an NTT at N is LR_ERR_NOT_NTT_FRIENDLY with lr_context_create's message; t == 0 and max_batch outside 1 .. 65535 are LR_ERR_ARG.
 * Two routes, the same bits, chosen once at creation: for 2^11 <= N <= 2^15 and t < 2^31 one kernel per direction with one workgroup per
 * plaintext and the transform over Z_t in LDS; otherwise (or with lr_options::bfv_encoder_unfused) the transform of contextT between
 * small scatter / lift / gather kernels.  The work is ordered on ctxQ's stream. */
typedef struct lr_bfv_encoder lr_bfv_encoder;
int lr_bfv_encoder_create(lr_context *ctxQ, uint64_t t, int max_batch, lr_bfv_encoder **out);
/* the same with explicit options; NULL = the options of ctxQ */
int lr_bfv_encoder_create_ex(lr_context *ctxQ, uint64_t t, int max_batch, const lr_options *opt, lr_bfv_encoder **out);
int lr_bfv_encoder_destroy(lr_bfv_encoder *enc);
/* host copies of indexMatrix[N] and deltaMont[|Q|], for parity tests */
int lr_bfv_encoder_tables(const lr_bfv_encoder *enc, uint64_t *index_matrix, uint64_t *delta_mont);
/* diagnostics: *fused = 1 when the handle runs the fused kernels, 0 on the composed route */
int lr_bfv_encoder_route(const lr_bfv_encoder *enc, int *fused);
/* EncodeUint / EncodeInt (:70-119): values = host [batch][n_values], n_values <= N (more: LR_ERR_SHAPE, the reference panics); slot i goes
 * to coefficient indexMatrix[i], the slots from n_values on are zero; pt over all of Q, coefficient domain, of the same batch
 * (batch != the poly's or > max_batch, or fewer than |Q| limbs: LR_ERR_SHAPE; a poly of another context: LR_ERR_ARG).  Uint values are
 * taken modulo t, Int values map to their residue in [0, t) (the reference's t + c for -t <= c < 0).  The values are staged through a
 * pinned buffer of the handle: the caller's array is free on return, the encoding is asynchronous. */
int lr_bfv_encode_uint(lr_bfv_encoder *enc, const uint64_t *values, size_t n_values, int batch, lr_poly *pt);
int lr_bfv_encode_int(lr_bfv_encoder *enc, const int64_t *values, size_t n_values, int batch, lr_poly *pt);
/* DecodeUint / DecodeInt (:139-182): values = host [batch][N]; DecodeInt subtracts t from the slots above t >> 1.  Synchronises. */
int lr_bfv_decode_uint(lr_bfv_encoder *enc, const lr_poly *pt, int batch, uint64_t *values);
int lr_bfv_decode_int(lr_bfv_encoder *enc, const lr_poly *pt, int batch, int64_t *values);
/* the same on slots in device memory ([batch][n_values] / [batch][N] words, uint64 or, with is_signed, int64): stream-ordered, no host copy */
int lr_bfv_encode_device(lr_bfv_encoder *enc, const void *device_values, size_t n_values, int batch, int is_signed, lr_poly *pt);
int lr_bfv_decode_device(lr_bfv_encoder *enc, const lr_poly *pt, int batch, int is_signed, void *device_values);

/* bfv.Encryptor (bfv/encryptor.go:100-345) for a batch of ciphertexts, device-resident, after the sampling.  lr_bfv_encryptor owns what
 * newEncryptor builds (:100-119): NewFastBasisExtender(contextQ, contextP), three pool polys over Q||P for max_batch ciphertexts, the
 * matrixTernaryMontgomery rows of every limb (ring/ring_context.go:119-122) and a pinned staging buffer.  ctxP == NULL is the reference's
 * "modulus P is empty": only the fast forms work (fast = 0 is LR_ERR_ARG).  max_batch outside 1 .. 65535, N < 8 (a bit plane is N / 8
 * bytes) and a ctxP on another device or of another N are LR_ERR_ARG.  The work is ordered on ctxQ's stream.
 * The randomness is the samplers' decisions in compact form, N / 4 + 2 N bytes per public-key ciphertext instead of three polys:
 *   u_coeff_bits, u_sign_bits  [batch][N / 8]: randomBytesCoeffs / randomBytesSign of sampleTernary at p = 0.5
 *                              (ring/ternarySampler.go:157-177); coefficient i uses bit i & 7 of byte i >> 3, and
 *                              index = (coeff & (sign ^ 1)) | ((sign & coeff) << 1) selects {0, MForm(1), MForm(q_j - 1)};
 *   e0, e1, e                  [batch][N]: per coefficient the Gaussian sampler's magnitude in the low 7 bits and its sign in bit 7; the
 *                              residue is the reference's (ring/gaussianSampler.go:247): sign 1 -> coeff, sign 0 -> q_j - coeff.
 * Keys are per-call arguments: polys of ctxQ in NTT + Montgomery form with |Q| + |P| limbs in contextQP's order (fast: |Q| suffice), of
 * the call's batch or of batch 1.  pt, out_c0, out_c1: over all of Q, coefficient domain, of the call's batch (pt may have batch 1);
 * out_c0 == out_c1 is LR_ERR_ARG, pt is not an output.  batch < 1, > max_batch or != the polys': LR_ERR_SHAPE; too few limbs:
 * LR_ERR_SHAPE; a poly of another context: LR_ERR_ARG.
 * lr_bfv_encrypt_pk = pkEncryptor.encrypt: fast = 0 is :194-216 (u -> NTT over Q||P, the two products with the key, InvNTT, Add of the
 * sampled polys, ModDownPQ(|Q| - 1), + pt on component 0), fast = 1 is :173-190 over Q alone without the ModDown (the reference leaves
 * that result in its pool, v1.3.1; here it is the ciphertext).
 * lr_bfv_encrypt_sk = skEncryptor.encrypt (:306-345) with crp the uniform poly in the NTT domain (over Q||P, fast: over Q), which is read
 * only: Neg(MulCoeffsMontgomery(crp, sk)), InvNTT of that and of crp, SampleAndAdd on the first, (fast = 0) ModDownPQ of both, + pt.
 * The host forms stage the bytes through the pinned buffer: the caller's arrays are free on return, the call is asynchronous.  The
 * _device forms take the same bytes in device memory: stream-ordered, no host copy, no synchronisation.
 * lr_options::no_epilogue selects the reference's call-by-call shape (the samplers expand into pool polys, then one launch per Context
 * call); both shapes give the same bits. */
typedef struct lr_bfv_encryptor lr_bfv_encryptor;
int lr_bfv_encryptor_create(lr_context *ctxQ, lr_context *ctxP, int max_batch, lr_bfv_encryptor **out);
/* the same with explicit options; NULL = the options of ctxQ */
int lr_bfv_encryptor_create_ex(lr_context *ctxQ, lr_context *ctxP, int max_batch, const lr_options *opt, lr_bfv_encryptor **out);
int lr_bfv_encryptor_destroy(lr_bfv_encryptor *enc);
int lr_bfv_encrypt_pk(lr_bfv_encryptor *enc, int fast, const lr_poly *pk0, const lr_poly *pk1, const uint8_t *u_coeff_bits,
                      const uint8_t *u_sign_bits, const uint8_t *e0, const uint8_t *e1, const lr_poly *pt, int batch, lr_poly *out_c0,
                      lr_poly *out_c1);
int lr_bfv_encrypt_sk(lr_bfv_encryptor *enc, int fast, const lr_poly *sk, const lr_poly *crp, const uint8_t *e, const lr_poly *pt, int batch,
                      lr_poly *out_c0, lr_poly *out_c1);
int lr_bfv_encrypt_pk_device(lr_bfv_encryptor *enc, int fast, const lr_poly *pk0, const lr_poly *pk1, const void *u_coeff_bits,
                             const void *u_sign_bits, const void *e0, const void *e1, const lr_poly *pt, int batch, lr_poly *out_c0,
                             lr_poly *out_c1);
int lr_bfv_encrypt_sk_device(lr_bfv_encryptor *enc, int fast, const lr_poly *sk, const lr_poly *crp, const void *e, const lr_poly *pt,
                             int batch, lr_poly *out_c0, lr_poly *out_c1);
/* bfv.Decryptor (bfv/decryptor.go:28-75).  lr_bfv_decrypt = decryptor.Decrypt of ct[0 .. degree] (degree >= 0; negative: LR_ERR_ARG):
 * NTT of every component (components that lie back to back in memory share a launch), Horner at sk with the reference's i & 7 == 7
 * reduction cadence, InvNTT.  ct[i] and pt_out: over all of Q, coefficient domain, of the given batch -- what lr_bfv_mul writes and
 * lr_bfv_decode_uint reads; sk in NTT + Montgomery form, its first |Q| limbs are read (a key over Q||P works), batch 1 or the call's.
 * pt_out may be ct[degree]; the inputs are not modified otherwise.  Refusals as above.  The handle's options are ctxQ's. */
typedef struct lr_bfv_decryptor lr_bfv_decryptor;
int lr_bfv_decryptor_create(lr_context *ctxQ, int max_batch, lr_bfv_decryptor **out);
int lr_bfv_decryptor_destroy(lr_bfv_decryptor *dec);
int lr_bfv_decrypt(lr_bfv_decryptor *dec, const lr_poly *const *ct, int degree, const lr_poly *sk, lr_poly *pt_out, int batch);

/* ckks.Encoder (ckks/encoder.go:10-226) for a batch of plaintexts, device-resident, bit for bit the reference compiled for amd64 (no
 * multiply-add fused, a complex product is (ac - bd, ad + bc)).  lr_ckks_encoder owns what ckks.NewEncoder builds (:31-69): rotGroup
 * (5^j mod m for j < m / 4, m = 2 N; the upper half of its m / 2 entries stays zero as in the reference) and the root table
 * roots[0 .. m] -- the caller's (cos, sin) pairs, 2 (m + 1) doubles, so that a Go caller passes the table Go's math.Cos / math.Sin gave
 * it; NULL = filled with the host libm from the reference's expression 2 * 3.141592653589793 * i / m, roots[m] = roots[0] -- plus the
 * per-level CRT tables of Decode, a pool of max_batch polys and a pinned staging buffer.  max_batch outside 1 .. 65535 is LR_ERR_ARG, and
 * so is a Q of more than 2048 bits (32 words in the decoder's multi-word CRT).
 * Two routes, the same bits: slots <= 2^13 run one workgroup per plaintext with the special FFT in LDS (Encode's scale-up in the same
 * kernel from batch 256 on, as a grid-wide kernel of its own below); larger slot counts, and every
 * slot count with lr_options::ckks_encoder_tiled, run the wide stages as streaming kernels and the others in LDS tiles.
 * values = [batch][slots] complex128 as (re, im) pairs; slots a power of two in 1 .. N / 2 (else LR_ERR_ARG: the reference's own check
 * at :84 is vacuous); scale finite and positive (else LR_ERR_ARG).  pt = a poly of ctxQ in the NTT domain with at least level + 1 limbs
 * and the given batch (what lr_ckks_encrypt_pk takes and lr_ckks_decrypt returns); limbs above level are not touched.  batch != the
 * poly's or > max_batch, too few limbs or a level outside 0 .. |Q| - 1: LR_ERR_SHAPE; a poly of another context: LR_ERR_ARG.
 * Encode (:78-116): invfft, scatter with gap = (N / 2) / slots, scaleUpVecExact (ckks/utils.go:51-98), NTTLvl(level).  Outside the
 * reference's defined domain the device does this: a coefficient x with scale x == 2^64 encodes as 0; a negative x with
 * |scale x| + 0.5 >= 2^64 as q_j minus the low 64 bits of the truncated integer, reduced; NaN and +-Inf coefficients as 0 (q_j for -Inf).
 * Decode (:119-168): InvNTTLvl(level), CRT over limbs 0 .. level, centring at Q_level >> 1, the exact integer to double as
 * big.Float.SetInt(..).Float64() (nearest-even, +-Inf from 2^1024), an IEEE division by scale, fft.
 * The work is ordered on ctxQ's stream.  The host-value calls stage through the pinned buffer: Encode is asynchronous and the
 * caller's array is free on return; Decode synchronises. */
typedef struct lr_ckks_encoder lr_ckks_encoder;
int lr_ckks_encoder_create(lr_context *ctxQ, int max_batch, const double *roots, lr_ckks_encoder **out);
/* the same with explicit options; NULL = the options of ctxQ */
int lr_ckks_encoder_create_ex(lr_context *ctxQ, int max_batch, const double *roots, const lr_options *opt, lr_ckks_encoder **out);
int lr_ckks_encoder_destroy(lr_ckks_encoder *enc);
/* host copies of rotGroup[m / 2] and roots[2 (m + 1)], for parity tests */
int lr_ckks_encoder_tables(const lr_ckks_encoder *enc, uint64_t *rot_group, double *roots);
/* diagnostics: *fused = 1 when a call with this slot count runs the fused kernels, 0 on the tiled route */
int lr_ckks_encoder_route(const lr_ckks_encoder *enc, int slots, int *fused);
int lr_ckks_encode(lr_ckks_encoder *enc, const double *values, int slots, int level, double scale, int batch, lr_poly *pt);
int lr_ckks_decode(lr_ckks_encoder *enc, const lr_poly *pt, int slots, int level, double scale, int batch, double *values);
/* the same on slot values in device memory ([batch][slots] complex128): stream-ordered, no host copy, no synchronisation */
int lr_ckks_encode_device(lr_ckks_encoder *enc, const void *device_values, int slots, int level, double scale, int batch, lr_poly *pt);
int lr_ckks_decode_device(lr_ckks_encoder *enc, const lr_poly *pt, int slots, int level, double scale, int batch, void *device_values);

/* ckks.Encryptor (ckks/encryptor.go:100-362) for a batch of ciphertexts, device-resident, after the sampling.  lr_ckks_encryptor owns what
 * newEncryptor builds (:100-119): NewFastBasisExtender(contextQ, contextP), three pool polys over Q||P for max_batch ciphertexts, the
 * matrixTernaryMontgomery rows of every limb (ring/ring_context.go:119-122) and a pinned staging buffer.  ctxP == NULL is the reference's
 * "modulus P is empty": only the fast forms work (fast = 0 is LR_ERR_ARG).  max_batch outside 1 .. 65535, N < 8 (a bit plane is N / 8
 * bytes) and a ctxP on another device or of another N are LR_ERR_ARG.  The work is ordered on ctxQ's stream.
 * The randomness is exactly lr_bfv_encryptor's: u_coeff_bits, u_sign_bits [batch][N / 8] (sampleTernary at p = 0.5), e0, e1, e [batch][N]
 * (magnitude in bits 0-6, sign in bit 7; the residue is ring/gaussianSampler.go:247: sign 1 -> coeff, sign 0 -> q_j - coeff) -- N / 4 + 2 N
 * bytes per public-key ciphertext instead of the three polys over Q||P that lr_ckks_encrypt_pk takes.
 * pt, out_c0, out_c1: polys of ctxQ in the NTT domain with at least level + 1 limbs, as lr_ckks_encode writes them and lr_ckks_decrypt
 * reads them; limbs above level are not touched.  Keys: polys of ctxQ in NTT + Montgomery form with |Q| + |P| limbs in contextQP's order
 * (fast: |Q| suffice).  Keys and pt have batch 1 or the call's batch.  crp: the uniform poly in the NTT domain, over Q||P (fast: over Q),
 * of the call's batch, read only (crp as an output is LR_ERR_ARG).  out_c0 == out_c1 is LR_ERR_ARG; a poly of another context is
 * LR_ERR_ARG; batch < 1, > max_batch or != the polys', too few limbs, or a level outside 0 .. |Q| - 1: LR_ERR_SHAPE.
 * encrypt_pk = pkEncryptor.encrypt (:179-237).
 *   fast = 1 (:187-200, :234): u expanded then NTT, e_k expanded then NTT, ct_k = CRed(MRed(u, pk_k) + e_k), + pt on component 0, all over
 *   limbs 0 .. level: below the top level the natural restriction of the reference's lines to those limbs.
 *   fast = 0 (:204-234): for the same decisions the bits of lr_ckks_encrypt_pk fed the expanded polys, at every level: u -> NTT, the two
 *   products and InvNTT over all of Q||P, SampleAndAdd on every row, ModDownPQ(level) -- which reads its "P part" at rows level + 1 ..
 *   level + |P| of the pool poly (ring_basis_extension.go:256) -- NTT over limbs 0 .. level, + pt.  The rows ModDownPQ reads are the
 *   special primes' only at level = |Q| - 1: below it the call follows the reference's lines literally and the result is not a
 *   ciphertext of pt (the reference itself only runs at the top level: its Context.NTT at :229 walks every modulus of contextQ).
 * encrypt_sk = skEncryptor.encrypt (:318-362).
 *   fast = 1 (:324-330, :359): ct0 = CRed(CRed(Neg(MRed(crp, sk)) + NTT(e)) + pt), ct1 = crp, over limbs 0 .. level (Neg of 0 is q_j, as
 *   in the reference).
 *   fast = 0 (:337-359): Neg(MRed(crp, sk)) over Q||P, InvNTT, SampleAndAdd, ModDownPQ(level) as above, NTT, + pt; ct1 =
 *   ModDownNTTPQ(level, crp), which reads its P part at rows |Q| .. (ring_basis_extension.go:163-190) and runs here on a copy of those
 *   rows, so that crp stays intact.  Below the top level ct1 is therefore round(crp / P) over limbs 0 .. level, while ct0 is what the
 *   literal ModDownPQ gives: only level = |Q| - 1 yields a ciphertext of pt.
 * The host forms stage the bytes through the pinned buffer: the caller's arrays are free on return, the call is asynchronous.  The
 * _device forms take the same bytes in device memory: stream-ordered, no host copy, no synchronisation.
 * lr_options::no_epilogue selects the reference's call-by-call shape (the samplers expand into pool polys, then one launch per Context
 * call); both shapes give the same bits. */
typedef struct lr_ckks_encryptor lr_ckks_encryptor;
int lr_ckks_encryptor_create(lr_context *ctxQ, lr_context *ctxP, int max_batch, lr_ckks_encryptor **out);
/* the same with explicit options; NULL = the options of ctxQ */
int lr_ckks_encryptor_create_ex(lr_context *ctxQ, lr_context *ctxP, int max_batch, const lr_options *opt, lr_ckks_encryptor **out);
int lr_ckks_encryptor_destroy(lr_ckks_encryptor *enc);
int lr_ckks_encryptor_encrypt_pk(lr_ckks_encryptor *enc, int fast, int level, const lr_poly *pk0, const lr_poly *pk1,
                                 const uint8_t *u_coeff_bits, const uint8_t *u_sign_bits, const uint8_t *e0, const uint8_t *e1,
                                 const lr_poly *pt, int batch, lr_poly *out_c0, lr_poly *out_c1);
int lr_ckks_encryptor_encrypt_sk(lr_ckks_encryptor *enc, int fast, int level, const lr_poly *sk, const lr_poly *crp, const uint8_t *e,
                                 const lr_poly *pt, int batch, lr_poly *out_c0, lr_poly *out_c1);
int lr_ckks_encryptor_encrypt_pk_device(lr_ckks_encryptor *enc, int fast, int level, const lr_poly *pk0, const lr_poly *pk1,
                                        const void *u_coeff_bits, const void *u_sign_bits, const void *e0, const void *e1,
                                        const lr_poly *pt, int batch, lr_poly *out_c0, lr_poly *out_c1);
int lr_ckks_encryptor_encrypt_sk_device(lr_ckks_encryptor *enc, int fast, int level, const lr_poly *sk, const lr_poly *crp, const void *e,
                                        const lr_poly *pt, int batch, lr_poly *out_c0, lr_poly *out_c1);

/* ckks.KeyGenerator and bfv.KeyGenerator (ckks/keygen.go:79-494, bfv/keygen.go:70-441) for a batch of keys, device-resident, after the
 * sampling.  lr_keygen owns what NewKeyGenerator builds -- a pool over Q||P -- plus MForm(P mod q_j), the matrixTernaryMontgomery rows of
 * every limb and a pinned staging buffer.  ctxP == NULL is the reference's "modulus P is empty": only lr_keygen_secret_key and
 * lr_keygen_public_key work, over Q (the three switching-key entry points are LR_ERR_ARG).  max_batch outside 1 .. 65535, N < 8 (a bit
 * plane is N / 8 bytes) and a ctxP on another device or of another N are LR_ERR_ARG.  The work is ordered on ctxQ's stream.
 * The randomness is exactly lr_bfv_encryptor's: coeff_bits, sign_bits [batch][N / 8] (coefficient i uses bit i & 7 of byte i >> 3, and
 * index = (coeff & (sign ^ 1)) | ((sign & coeff) << 1) selects {0, MForm(1), MForm(q_j - 1)} -- what sampleTernary ends in at p = 1/3, at
 * any p and in the sparse sampler alike); e [..][N] bytes per sampled poly, magnitude in bits 0-6, sign in bit 7 (the residue is
 * ring/gaussianSampler.go:247: sign 1 -> coeff, sign 0 -> q_j - coeff).  Both Gaussian samplers are bound to contextQP
 * (ckks/ckks.go:81, bfv/bfv.go:70), so one byte decides a coefficient on every row of Q||P.  The uniform polys are the caller's.
 * Every poly is a poly of ctxQ in NTT + Montgomery form with |Q| + |P| limbs in contextQP's order.
 * lr_keygen_secret_key = GenSecretKey (ckks/keygen.go:97-113): SampleTernaryMontgomeryNTTNew into sk_out, batch polys.
 * lr_keygen_public_key = GenPublicKey (:138-151): pk0_out = Neg(MulCoeffsMontgomeryAndAdd(sk, pk1, SampleNTT(e))) (Neg of 0 is q_j, as in
 *   the reference); pk1 = the caller's uniform poly, read only; sk has batch 1 or the call's; e = [batch][N].
 * The three switching-key entry points are newSwitchingKey (ckks/keygen.go:282-338, bfv/keygen.go:285-333) for n_keys keys.  evks = n_keys
 *   polys in the layout lr_ckks_switch_keys reads: batch 2 beta (beta = ceil(|Q| / |P|)), member 2 i = evakey[i][0], member 2 i + 1 =
 *   evakey[i][1].  The odd members hold the caller's uniform a on entry and are not written (the reference samples a straight into the
 *   key too); the even members are outputs: evakey[i][0] = CRed(CRed(MForm(NTT(e_i)) + [row in digit i] P skIn) + (q_j - MRed(a_i, skOut))),
 *   digit i owning rows i |P| .. min((i + 1) |P|, |Q|) - 1.  e = [n_keys][beta][N].  The keys are read through the pointer array: they
 *   need not be contiguous.  The two schemes' lines -- P multiplied in before or after the powers of sk, the digit loop broken at |Q| - 1
 *   or at |Q| + |P| - 1 -- give the same bits (every MRed is fully reduced, P skIn is zero on the rows of P), so one path serves both.
 *   lr_keygen_switching_keys = GenSwitchingKey (:247-258): skIn = sk_in, batch n_keys or 1; sk_out has batch n_keys or 1.
 *   lr_keygen_relin_keys = GenRelinKey: key i switches from sk^(i + 2); n_powers = 1 is ckks/keygen.go:192-205, n_powers = maxDegree is
 *     bfv/keygen.go:172-196.  sk has batch 1.
 *   lr_keygen_rotation_keys = genrotKey (ckks/keygen.go:487-494, bfv/keygen.go:429-441) for each Galois element: skIn =
 *     PermuteNTT(sk, galois_elements[k]).  sk has batch 1; the elements are read on the host during the call.
 * Refusals: LR_ERR_ARG: a null argument, a poly of another context, an output that shares memory with an input or with another output,
 * an even Galois element, a switching-key call on a handle without ctxP, ctxQ and ctxP on different streams at the time of a call
 * (every entry point of a handle with a ctxP: call lr_context_set_stream on both or on neither); LR_ERR_SHAPE: batch, n_keys or
 * n_powers < 1 or > max_batch, a poly with fewer than |Q| + |P| limbs, a poly whose batch differs from the call's (where batch 1 is not
 * allowed), a key whose batch is not 2 beta; LR_ERR_UNSUPPORTED, at creation: N > 2^30, more than 64 limbs in Q||P.
 * The host forms stage the bytes through the pinned buffer: the caller's arrays are free on return, the call is asynchronous.  The
 * _device forms take the same bytes in device memory: stream-ordered, no host copy, no synchronisation.
 * lr_options::no_epilogue selects the reference's call-by-call shape (one launch per Context call: MForm, Add on the digit's rows,
 * MulCoeffsMontgomeryAndSub, PermuteNTT, MulScalarBigint, MulCoeffsMontgomery); both shapes give the same bits. */
typedef struct lr_keygen lr_keygen;
int lr_keygen_create(lr_context *ctxQ, lr_context *ctxP, int max_batch, lr_keygen **out);
/* the same with explicit options; NULL = the options of ctxQ */
int lr_keygen_create_ex(lr_context *ctxQ, lr_context *ctxP, int max_batch, const lr_options *opt, lr_keygen **out);
int lr_keygen_destroy(lr_keygen *kg);
int lr_keygen_secret_key(lr_keygen *kg, const uint8_t *coeff_bits, const uint8_t *sign_bits, int batch, lr_poly *sk_out);
int lr_keygen_public_key(lr_keygen *kg, const lr_poly *sk, const uint8_t *e, int batch, lr_poly *pk0_out, const lr_poly *pk1);
int lr_keygen_switching_keys(lr_keygen *kg, const lr_poly *sk_in, const lr_poly *sk_out, const uint8_t *e, int n_keys, lr_poly *const *evks);
int lr_keygen_relin_keys(lr_keygen *kg, const lr_poly *sk, int n_powers, const uint8_t *e, lr_poly *const *evks);
int lr_keygen_rotation_keys(lr_keygen *kg, const lr_poly *sk, const uint64_t *galois_elements, int n_keys, const uint8_t *e,
                            lr_poly *const *evks);
int lr_keygen_secret_key_device(lr_keygen *kg, const void *coeff_bits, const void *sign_bits, int batch, lr_poly *sk_out);
int lr_keygen_public_key_device(lr_keygen *kg, const lr_poly *sk, const void *e, int batch, lr_poly *pk0_out, const lr_poly *pk1);
int lr_keygen_switching_keys_device(lr_keygen *kg, const lr_poly *sk_in, const lr_poly *sk_out, const void *e, int n_keys,
                                    lr_poly *const *evks);
int lr_keygen_relin_keys_device(lr_keygen *kg, const lr_poly *sk, int n_powers, const void *e, lr_poly *const *evks);
int lr_keygen_rotation_keys_device(lr_keygen *kg, const lr_poly *sk, const uint64_t *galois_elements, int n_keys, const void *e,
                                   lr_poly *const *evks);

/* Collective key switching of dckks and dbfv for a batch of ciphertexts, device-resident, after the sampling: CKSProtocol.GenShare
 * (dckks/keyswitching.go:62-94, dbfv/keyswitching.go:74-109), PCKSProtocol.GenShare (dckks/public_keyswitching.go:63-93,
 * dbfv/public_keyswitching.go:111-148), and AggregateShares / KeySwitch of all four (dckks/keyswitching.go:99-108,
 * dckks/public_keyswitching.go:99-113, dbfv/keyswitching.go:114-122, dbfv/public_keyswitching.go:154-165) as one n-ary fold.
 * lr_collective owns what the four New*Protocol constructors build: NewFastBasisExtender(contextQ, contextP), three pool polys over Q||P
 * for max_batch ciphertexts (tmp, share0tmp, share1tmp), MForm(P mod q_j), the matrixTernaryMontgomery rows of every limb and a pinned
 * staging buffer with its event.  ctxP is required (all four protocols divide by P): NULL is LR_ERR_ARG.  max_batch outside 1 .. 65535,
 * N < 8 (a bit plane is N / 8 bytes) and a ctxP on another device, of another N or on another stream are LR_ERR_ARG.  The work is ordered
 * on ctxQ's stream.
 * The randomness is exactly the encryptors': e, e0, e1 [batch][N] bytes (magnitude in bits 0-6, sign in bit 7; the residue is
 * ring/gaussianSampler.go:247: sign 1 -> coeff, sign 0 -> q_j - coeff), u_coeff_bits, u_sign_bits [batch][N / 8] (sampleTernary at
 * p = 0.5) -- N bytes per CKS share, N / 4 + 2 N per PCKS share.  The smudging sampler and the regular one differ only in which bytes the
 * caller draws.  A magnitude is at most 127: with the reference's bound int(6 sigma) that is sigma_smudge <= 21 (the reference's tests
 * use 6.36, its examples 3.19); larger magnitudes are outside this interface's domain.
 * Keys: polys of ctxQ in NTT + Montgomery form over Q||P in contextQP's order (|Q| limbs suffice for sk, sk_in and sk_out), of batch 1 or
 * the call's batch.  CKKS c1 and shares: NTT domain, at least level + 1 limbs; limbs above level are not touched.  BFV c1 and shares:
 * coefficient domain over all of Q.  Both of the call's batch.
 * lr_collective_ckks_cks_share: Sub over Q (:64), MulCoeffsMontgomeryLvl (:74), MulScalarBigintLvl by P (:76), SampleNTT over Q||P and
 *   AddLvl (:79-80), hP = the rows of P of the transformed noise (:82-88), ModDownSplitedNTTPQ(level) (:90).  A share at every level.
 *   Default shape: the noise is expanded on limbs 0 .. level and on the rows of P only, and only the rows of Q are transformed -- the
 *   ModDown transforms hP straight back (ring_basis_extension.go:199-201), so hP is the noise itself with its q_j of (0, sign 0) reduced
 *   to 0 -- then one pass CRed(MRed(MRed(c1, CRed(sk_in + q - sk_out)), MForm(P mod q_j)) + NTT(e)), then the ModDown.
 * lr_collective_bfv_cks_share (dbfv/keyswitching.go:76-105): NTT(c1), the same products, InvNTT, Sample over Q||P and Add over Q, hP = the
 *   sampled rows of P, ModDownSplitedPQ.  (0, sign 0) leaves the residue p_j itself in hP; the default shape writes 0 there, which changes
 *   no bit of the ModDown's output (pinned on the CPU, tests/test_oracle_collective.py); the call-by-call shape feeds p_j literally.
 * lr_collective_ckks_pcks_share (dckks/public_keyswitching.go:68-90): u -> NTT over Q||P, the products with pk0 and pk1, SampleNTT + Add
 *   of e0 and e1, two ModDownNTTPQ(level), MulCoeffsMontgomeryAndAddLvl(c1, sk) onto out0.  Default shape: everything in front of the
 *   ModDowns on limbs 0 .. level and the rows of P only (the rows a ModDownNTTPQ(level) reads).
 * lr_collective_bfv_pcks_share (dbfv/public_keyswitching.go:116-144): pkEncryptor.encrypt's steps through P (products, InvNTT,
 *   SampleAndAdd, two ModDownPQ(|Q| - 1)), then out0 += InvNTT(MRed(NTT(c1), sk)).
 * lr_collective_aggregate: acc = shares[0]; acc = CRed(acc + shares[k]) for k = 1 .. n_shares - 1 in this order; out = CRed(base + acc)
 *   if base is not NULL, else acc; over limbs 0 .. level.  n_shares = 1 and base = NULL is KeySwitch's Copy, base = ct[0] its Add.  One
 *   pass reads n_shares (+ 1) rows and writes one; more than 32 shares run as further passes over the running sum.  out may be base or
 *   any of the shares (AggregateShares(a, b, a)); a partial overlap is LR_ERR_ARG.  Every poly has the same batch, at most max_batch.
 * Refusals: LR_ERR_ARG: a null argument, a poly of another context, an output of a share call that shares memory with an input or with
 * the other output, ctxQ and ctxP on different streams at the time of a call; LR_ERR_SHAPE: batch < 1 or > max_batch, a poly with too few
 * limbs, a poly whose batch differs from the call's (where batch 1 is not allowed), a level outside 0 .. |Q| - 1, n_shares < 1;
 * LR_ERR_UNSUPPORTED, at creation: more than 64 limbs in Q||P.
 * The host forms stage the bytes through the pinned buffer: the caller's arrays are free on return, the call is asynchronous.  The
 * _device forms take the same bytes in device memory: kernels only on ctxQ's stream, no host copy, no synchronisation.
 * lr_options::no_epilogue selects the reference's call-by-call shape (one launch per Context call, every line over the rows the
 * reference walks); both shapes give the same bits. */
typedef struct lr_collective lr_collective;
int lr_collective_create(lr_context *ctxQ, lr_context *ctxP, int max_batch, lr_collective **out);
/* the same with explicit options; NULL = the options of ctxQ */
int lr_collective_create_ex(lr_context *ctxQ, lr_context *ctxP, int max_batch, const lr_options *opt, lr_collective **out);
int lr_collective_destroy(lr_collective *col);
int lr_collective_ckks_cks_share(lr_collective *col, int level, const lr_poly *sk_in, const lr_poly *sk_out, const lr_poly *c1,
                                 const uint8_t *e, int batch, lr_poly *share_out);
int lr_collective_bfv_cks_share(lr_collective *col, const lr_poly *sk_in, const lr_poly *sk_out, const lr_poly *c1, const uint8_t *e,
                                int batch, lr_poly *share_out);
int lr_collective_ckks_pcks_share(lr_collective *col, int level, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1,
                                  const lr_poly *c1, const uint8_t *u_coeff_bits, const uint8_t *u_sign_bits, const uint8_t *e0,
                                  const uint8_t *e1, int batch, lr_poly *out0, lr_poly *out1);
int lr_collective_bfv_pcks_share(lr_collective *col, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1, const lr_poly *c1,
                                 const uint8_t *u_coeff_bits, const uint8_t *u_sign_bits, const uint8_t *e0, const uint8_t *e1, int batch,
                                 lr_poly *out0, lr_poly *out1);
int lr_collective_ckks_cks_share_device(lr_collective *col, int level, const lr_poly *sk_in, const lr_poly *sk_out, const lr_poly *c1,
                                        const void *e, int batch, lr_poly *share_out);
int lr_collective_bfv_cks_share_device(lr_collective *col, const lr_poly *sk_in, const lr_poly *sk_out, const lr_poly *c1, const void *e,
                                       int batch, lr_poly *share_out);
int lr_collective_ckks_pcks_share_device(lr_collective *col, int level, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1,
                                         const lr_poly *c1, const void *u_coeff_bits, const void *u_sign_bits, const void *e0,
                                         const void *e1, int batch, lr_poly *out0, lr_poly *out1);
int lr_collective_bfv_pcks_share_device(lr_collective *col, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1, const lr_poly *c1,
                                        const void *u_coeff_bits, const void *u_sign_bits, const void *e0, const void *e1, int batch,
                                        lr_poly *out0, lr_poly *out1);
int lr_collective_aggregate(lr_collective *col, int level, const lr_poly *base /* may be NULL */, const lr_poly *const *shares, int n_shares,
                            lr_poly *out);

/* The collective Refresh of dckks and dbfv for a batch of ciphertexts, device-resident, after the sampling: RefreshProtocol.GenShares,
 * Aggregate, Decrypt, Recode and Recrypt of dckks/public_refresh.go (:43-95 after the drawing of the mask and the noise, :98, :103,
 * :108-139, :142-147) and GenShares, Aggregate, Decrypt, Recode, Recrypt, Finalize and lift of dbfv/public_refresh.go (:105-160, :163,
 * :169, :174-179, :182-190, :193-197, :199-205).
 * lr_refresh owns what the two NewRefreshProtocol constructors build: three pool polys over Q||P for max_batch ciphertexts, and with a
 * ctxP NewFastBasisExtender(contextQ, contextP), with t NewSimpleScaler(t, contextQ) and deltaMont; further 2^64 mod q_i, the constants
 * of Recode and a pinned staging buffer with its event.  ctxP = NULL or t = 0 make a handle for the CKKS entry points only: the two BFV
 * entry points then are LR_ERR_ARG.  max_batch outside 1 .. 65535, N < 8 and a ctxP on another device, of another N or on another stream
 * are LR_ERR_ARG; more than 64 limbs in Q||P is LR_ERR_UNSUPPORTED.  The work is ordered on ctxQ's stream.
 * Randomness, drawn by the caller.  e0, e1: [batch][N] bytes as for lr_collective (magnitude at most 127 in bits 0-6, sign in bit 7;
 * both references sample with sigma = 3.19, bound 19).  CKKS mask: what ring.RandInt(Q_levelStart / 2 nParties) gives per coefficient,
 * centred (:58-62), as a signed integer in two's complement on W little-endian 64-bit words, word planes [batch][W][N] (word w of
 * coefficient j of member b at (b W + w) N + j); W = ceil(bitlen(Q_levelStart) / 64) is what lr_refresh_mask_words reports.  Every W-word
 * value is in the domain and is reduced as the integer it is: out_i = big.Int.Mod(mask, q_i), Euclidean; nParties enters only the caller's
 * bound.  A Q_levelStart of more than 32 words (2048 bits) is LR_ERR_UNSUPPORTED in every CKKS call and in lr_refresh_mask_words.  BFV
 * mask: [batch][N] uint64, uniform below t (contextT.NewUniformPoly); lift is applied on the device, and a value >= t is fed to MRed as it
 * is.  _device forms: the CKKS mask aligned to 8 bytes, the BFV mask to 16, else LR_ERR_ARG.
 * sk: NTT + Montgomery form, batch 1 or the call's; |Q| limbs for CKKS, |Q| + |P| for BFV (it is read on the rows of P, :141).  Every
 * other poly has the call's batch.
 * lr_refresh_ckks_shares: share_decrypt = NTT(mask) + sk c1 + NTT(e0) on limbs 0 .. level_start (:66, :74, :78, :84-85), limbs above
 *   not touched; share_recrypt = -(NTT(mask) + sk crs + NTT(e1)) over all of Q (:68, :75, :81, :88-89, :92); every addition with its
 *   CRed in this order, Neg as q_i - x (a zero is stored as q_i).  c1: NTT domain, level_start + 1 limbs; crs: NTT domain, |Q| limbs.
 *   Default shape: the mask is reduced and transformed once over all of Q and its first level_start + 1 rows serve both shares; e0 is
 *   expanded on limbs 0 .. level_start only; one pass per row computes both shares.
 * lr_refresh_ckks_recode (:108-139): in, NTT domain, canonical residues on limbs 0 .. level_start -> out, NTT domain over all of Q, of
 *   v = the CRT of the input rows in [0, Q_ls), v >= Q_ls >> 1 => v -= Q_ls (Cmp gives 1 or 0), out_i = v mod q_i (Euclidean).  out may be
 *   in.  The integer is held as mixed-radix digits (Garner), never as words.  Default shape: rows 0 .. level_start of out are copied from
 *   in (v mod q_i is the input's residue there), only the new rows are computed and transformed.  level_start = |Q| - 1 is legal.
 * lr_refresh_ckks_finalize: Decrypt's AddLvl (:104), Recode, Recrypt's Add (:144) into out0 over all of Q; out0 may be c0.  ct[1] =
 *   crs.CopyNew() (:146) stays the caller's copy.
 * lr_refresh_bfv_shares: share_decrypt = ModDownSplitedPQ(P InvNTT(sk NTT(c1)) + e0 on Q, e0's rows of P) + lift(mask) (:116-137, :156);
 *   share_recrypt = ModDownPQ(InvNTT(-sk NTT(crs)) + e1 over Q||P) - lift(mask) (:140-149, :159).  c1 and the shares: coefficient domain,
 *   |Q| limbs; crs: coefficient domain, |Q| + |P| limbs.  Deviation: the reference's rfp.hP is never zeroed (cks.hP is,
 *   dbfv/keyswitching.go:108), so a second GenShares on one Go object accumulates unreduced noise; every call here behaves as the first
 *   call on a fresh RefreshProtocol.  (0, sign 0) leaves the residue p_j itself in hP; the default shape writes 0 there, which changes no
 *   bit of the ModDown's output (tests/test_oracle_refresh.py); the call-by-call shape feeds p_j literally.
 * lr_refresh_bfv_finalize: out0 = lift(SimpleScaler.Scale(c0 + share_decrypt)) + share_recrypt (:170, :177-178, :185), out1 =
 *   ModDownPQ(|Q| - 1, crs) (:188); out0 may be c0.
 * lr_refresh_aggregate: lr_collective_aggregate without a base, over limbs 0 .. level: Aggregate of both protocols for n_shares parties
 *   in their order; out may be any of the shares.
 * Every input is left unchanged.  Refusals: LR_ERR_ARG: a null argument, a poly of another context, an output that shares memory with an
 * input or the other output (but for the aliases named above), a misaligned _device mask, a BFV call on a CKKS-only handle, ctxQ and
 * ctxP on different streams at the time of a call; LR_ERR_SHAPE: batch < 1 or > max_batch, a poly with too few limbs, a poly whose batch
 * differs from the call's, a level outside 0 .. |Q| - 1, n_shares < 1; LR_ERR_UNSUPPORTED: the two named above.
 * Host forms stage mask and noise through the pinned buffer (the caller's arrays are free on return, the call is asynchronous); _device
 * forms take the same bytes in device memory: kernels only, no host copy, no synchronisation.  lr_options::no_epilogue selects the
 * reference's call-by-call shape; both shapes give the same bits. */
typedef struct lr_refresh lr_refresh;
int lr_refresh_create(lr_context *ctxQ, lr_context *ctxP /* NULL: CKKS only */, uint64_t t /* 0: CKKS only */, int max_batch, lr_refresh **out);
/* the same with explicit options; NULL = the options of ctxQ */
int lr_refresh_create_ex(lr_context *ctxQ, lr_context *ctxP, uint64_t t, int max_batch, const lr_options *opt, lr_refresh **out);
int lr_refresh_destroy(lr_refresh *r);
int lr_refresh_mask_words(const lr_refresh *r, int level_start, int *words);
int lr_refresh_ckks_shares(lr_refresh *r, int level_start, const lr_poly *sk, const lr_poly *c1, const lr_poly *crs, const uint64_t *mask,
                           const uint8_t *e0, const uint8_t *e1, int batch, lr_poly *share_decrypt, lr_poly *share_recrypt);
int lr_refresh_ckks_shares_device(lr_refresh *r, int level_start, const lr_poly *sk, const lr_poly *c1, const lr_poly *crs, const void *mask,
                                  const void *e0, const void *e1, int batch, lr_poly *share_decrypt, lr_poly *share_recrypt);
int lr_refresh_ckks_recode(lr_refresh *r, int level_start, const lr_poly *in, lr_poly *out);
int lr_refresh_ckks_finalize(lr_refresh *r, int level_start, const lr_poly *c0, const lr_poly *share_decrypt, const lr_poly *share_recrypt,
                             lr_poly *out0);
int lr_refresh_bfv_shares(lr_refresh *r, const lr_poly *sk, const lr_poly *c1, const lr_poly *crs, const uint64_t *mask, const uint8_t *e0,
                          const uint8_t *e1, int batch, lr_poly *share_decrypt, lr_poly *share_recrypt);
int lr_refresh_bfv_shares_device(lr_refresh *r, const lr_poly *sk, const lr_poly *c1, const lr_poly *crs, const void *mask, const void *e0,
                                 const void *e1, int batch, lr_poly *share_decrypt, lr_poly *share_recrypt);
int lr_refresh_bfv_finalize(lr_refresh *r, const lr_poly *c0, const lr_poly *crs, const lr_poly *share_decrypt, const lr_poly *share_recrypt,
                            lr_poly *out0, lr_poly *out1);
int lr_refresh_aggregate(lr_refresh *r, int level, const lr_poly *const *shares, int n_shares, lr_poly *out);

/* The collective key setup of dckks and dbfv for a batch of parties, device-resident, after the sampling: CKGProtocol.GenShare
 * (dbfv/publickey_gen.go:54-57), the rounds and GenRelinearizationKey of RKGProtocol (dbfv/relinkey_gen.go:215-355) and of
 * RKGProtocolNaive (dbfv/relinkey_gen_naive.go:59-200), RTGProtocol.genShare and Finalize (dbfv/rotkey_gen.go:139-215), and every
 * Aggregate* of the four as one n-ary fold.  The dckks twins compute the same lines except where noted.  lr_setup owns what the four
 * New*Protocol constructors build -- polypool / tmpPoly over Q||P -- plus a pool for the transformed samples of one pass of up to 32
 * parties, MForm(P mod q_j), the matrixTernaryMontgomery rows of every limb and a pinned staging buffer with its event.  ctxP == NULL is
 * the reference's "P is empty": only lr_setup_ckg_share and lr_setup_aggregate (batch 1) work, over Q; every other entry point is
 * LR_ERR_ARG.  max_batch outside 1 .. 65535, N < 8 (a bit plane is N / 8 bytes) and a ctxP on another device or of another N are
 * LR_ERR_ARG.  The work is ordered on ctxQ's stream.
 * Every poly is a poly of ctxQ with |Q| + |P| limbs in contextQP's order, in the NTT domain.  sk, u (lr_keygen_secret_key is
 * NewEphemeralKey's SampleTernaryMontgomeryNTTNew) and pk0, pk1 are in Montgomery form, as lr_keygen writes them; crs and crp are used as
 * the reference uses them, without an MForm, until a finalize step says otherwise.  beta = ceil(|Q| / |P|); digit i owns rows i |P| ..
 * min((i + 1) |P|, |Q|) - 1 (the reference's digit loop with its break; its three spellings of the break give the same rows).
 * Layout: a share of beta polys is one lr_poly of batch beta, member i = share[i]; a share of beta pairs is one lr_poly of batch 2 beta,
 * member 2 i = [i][0], member 2 i + 1 = [i][1] -- exactly the key image lr_ckks_switch_keys and lr_bfv_relinearize read, so the finalize
 * steps write keys in place.  crp is one poly of batch beta, read only.  A call serves n_parties parties (RTG: n_keys Galois elements),
 * 1 <= n <= max_batch; sk and u have batch n, or batch 1 where one key serves the call; the outputs come through a pointer array and need
 * not be contiguous.  More than 32 parties run as further passes over the pool.
 * Randomness, drawn by the caller in the order the reference draws it: a noise poly is [N] bytes, magnitude (at most 127) in bits 0-6,
 * sign in bit 7 (ring/gaussianSampler.go:247: sign 1 -> coeff, sign 0 -> q_j - coeff), one byte deciding the coefficient on every row of
 * Q||P; a ternary poly is two bit planes of [N / 8] bytes as for lr_keygen_secret_key.
 * lr_setup_ckg_share: share = CRed(NTT(e) + (q - MRed(sk, crs))) on every row; e = [batch][N]; sk and crs have batch 1 or the call's.
 *   GenPublicKey is a Set and needs no call: the aggregate share is pk0, crs is pk1.
 * lr_setup_rkg_round1 (:215-259): share[i] = NTT(e_i); on the rows digit i owns CRed(. + InvMForm(MulScalarBigint(sk, P))); on every row
 *   CRed(. + (q - MRed(u, crp[i]))).  e = [n][beta][N].
 * lr_setup_rkg_round2 (:277-299): [i][0] = CRed(MRed(round1[i], sk) + NTT(e1_i)), [i][1] = CRed(NTT(e2_i) + MRed(sk, crp[i])); e =
 *   [n][beta][2][N], e1_i before e2_i; round1 = the aggregate, one poly of batch beta shared by the call.
 * lr_setup_rkg_round3 (:322-333): share[i] = CRed(NTT(e_i) + MRed(CRed((u + q) - sk), round2[i][1])); e = [n][beta][N]; round2 = the
 *   aggregate, batch 2 beta.
 * lr_setup_rkg_key (:343-355): evk[i][0] = MForm(CRed(round2[i][0] + round3[i])), evk[i][1] = MForm(round2[i][1]); evk_out may be round2
 *   itself (in place).
 * lr_setup_rkg_naive_round1 (relinkey_gen_naive.go:59-110): [i][0] = CRed(CRed(NTT(e_i0) + [rows of digit i] InvMForm(P sk)) + MRed(pk0,
 *   u_i)), [i][1] = CRed(NTT(e_i1) + MRed(pk1, u_i)), u_i = SampleTernaryMontgomeryNTT(0.5) over Q||P; e = [n][beta][2][N] (the reference
 *   draws the noise of every digit before the first ternary), the planes [n][beta][N / 8].  scheme = LR_SETUP_BFV: these lines.  scheme =
 *   LR_SETUP_CKKS: dckks/relinkey_gen_naive.go:73-75 draws both noise polys into shareOut[i][0] -- the second draw overwrites the first --
 *   and shareOut[i][1] gets no noise, MulCoeffsMontgomeryAndAdd landing on whatever the share held.  The device takes the same
 *   [beta][2][N] bytes, uses e[i][1] for [i][0] and nothing for [i][1], and treats the share as freshly allocated (zero): every call
 *   behaves as the first call on shares from AllocateShares, the convention lr_refresh set for rfp.hP.  Another scheme is LR_ERR_ARG.
 * lr_setup_rkg_naive_round2 (:135-166): [i][c] = CRed(CRed(MRed(round1[i][c], sk) + MRed(pk_c, v_i)) + NTT(e_ic)); the same in dckks.
 * lr_setup_rkg_naive_key (:187-200): MForm of both halves; evk_out may be round2 itself.  pk0, pk1: batch 1.
 * lr_setup_rtg_share (rotkey_gen.go:139-184) for Galois element g_k: share_k[i] = NTT(e_ki); on the rows digit i owns CRed(. +
 *   InvMForm(MulScalarBigint(PermuteNTT(sk, g_k), P))); on every row MForm(CRed(. + (q - MRed(crp[i], sk)))).  e = [n_keys][beta][N]; sk
 *   has batch 1; the elements are read on the host during the call and reduced modulo 2 N.  The map from (rotation type, k) to an element
 *   stays with the caller, as for lr_keygen_rotation_keys.
 * lr_setup_rtg_key (:205-215): member 2 i = share[i], member 2 i + 1 = MForm(crp[i]).
 * lr_setup_aggregate: acc = shares[0]; acc = CRed(acc + shares[k]) for k = 1 .. n_shares - 1 in this order, over ALL rows of Q||P, for
 *   polys of batch 1, beta or 2 beta (all the same): every Aggregate* body of the four protocols.  One pass reads up to 32 shares; more
 *   run as further passes over the running sum.  out may be one of the shares; a partial overlap is LR_ERR_ARG.
 * Every input is left unchanged.  Refusals: LR_ERR_ARG: a null argument, a poly of another context, an output that overlaps an input or
 * another output (but for the two in-place cases above), ctxQ and ctxP on different streams at the time of a call, an even Galois
 * element, an unknown scheme, a P-protocol on a handle without ctxP; LR_ERR_SHAPE: n < 1 or n > max_batch, n_shares < 1, a poly with
 * fewer than |Q| + |P| limbs, a share whose batch is not beta or 2 beta as required, a key poly whose batch is neither 1 nor n;
 * LR_ERR_UNSUPPORTED, at creation: more than 64 limbs in Q||P; N > 2^30 (the RTG kernel's Galois index is computed in 32 bits).  The
 * second cannot be reached today: no context of such a degree can be made (its tables alone are 16 GiB per limb), so no test tries it.
 * Memory: the pool is sized for the widest call, the naive rounds: 3 beta min(max_batch, 32) + 1 polys over Q||P (two noise polys and a
 * ternary per party and digit, and polypool), plus max(2 beta, 1) for the fold -- at PN15QP880 (21 rows, beta 6) 5.25 MiB per poly, about
 * 3.0 GiB for max_batch >= 32 and 163 MiB for max_batch = 1; the staging buffer adds max_batch beta (2 N + N / 4) bytes, pinned and on
 * the device.  A caller that makes one handle per protocol object (the Go overlays do, with max_batch 1) pays the small figure each.
 * The host forms stage the bytes through the pinned buffer: the caller's arrays are free on return, the call is asynchronous.  The
 * _device forms take the same bytes in device memory: kernels only, no host copy, no synchronisation.
 * lr_options::no_epilogue selects the reference's call-by-call shape (one launch per Context call; a sampler's write into a share is a
 * copy out of the pool); both shapes give the same bits. */
typedef struct lr_setup lr_setup;
enum { LR_SETUP_BFV = 0, LR_SETUP_CKKS = 1 };
int lr_setup_create(lr_context *ctxQ, lr_context *ctxP, int max_batch, lr_setup **out);
/* the same with explicit options; NULL = the options of ctxQ */
int lr_setup_create_ex(lr_context *ctxQ, lr_context *ctxP, int max_batch, const lr_options *opt, lr_setup **out);
int lr_setup_destroy(lr_setup *s);
int lr_setup_ckg_share(lr_setup *s, const lr_poly *sk, const lr_poly *crs, const uint8_t *e, int batch, lr_poly *share_out);
int lr_setup_ckg_share_device(lr_setup *s, const lr_poly *sk, const lr_poly *crs, const void *e, int batch, lr_poly *share_out);
int lr_setup_rkg_round1(lr_setup *s, const lr_poly *u, const lr_poly *sk, const lr_poly *crp, const uint8_t *e, int n_parties,
                        lr_poly *const *shares);
int lr_setup_rkg_round1_device(lr_setup *s, const lr_poly *u, const lr_poly *sk, const lr_poly *crp, const void *e, int n_parties,
                               lr_poly *const *shares);
int lr_setup_rkg_round2(lr_setup *s, const lr_poly *round1, const lr_poly *sk, const lr_poly *crp, const uint8_t *e, int n_parties,
                        lr_poly *const *shares);
int lr_setup_rkg_round2_device(lr_setup *s, const lr_poly *round1, const lr_poly *sk, const lr_poly *crp, const void *e, int n_parties,
                               lr_poly *const *shares);
int lr_setup_rkg_round3(lr_setup *s, const lr_poly *round2, const lr_poly *u, const lr_poly *sk, const uint8_t *e, int n_parties,
                        lr_poly *const *shares);
int lr_setup_rkg_round3_device(lr_setup *s, const lr_poly *round2, const lr_poly *u, const lr_poly *sk, const void *e, int n_parties,
                               lr_poly *const *shares);
int lr_setup_rkg_key(lr_setup *s, const lr_poly *round2, const lr_poly *round3, lr_poly *evk_out);
int lr_setup_rkg_naive_round1(lr_setup *s, int scheme, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1, const uint8_t *e,
                              const uint8_t *u_coeff_bits, const uint8_t *u_sign_bits, int n_parties, lr_poly *const *shares);
int lr_setup_rkg_naive_round1_device(lr_setup *s, int scheme, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1, const void *e,
                                     const void *u_coeff_bits, const void *u_sign_bits, int n_parties, lr_poly *const *shares);
int lr_setup_rkg_naive_round2(lr_setup *s, const lr_poly *round1, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1,
                              const uint8_t *v_coeff_bits, const uint8_t *v_sign_bits, const uint8_t *e, int n_parties,
                              lr_poly *const *shares);
int lr_setup_rkg_naive_round2_device(lr_setup *s, const lr_poly *round1, const lr_poly *sk, const lr_poly *pk0, const lr_poly *pk1,
                                     const void *v_coeff_bits, const void *v_sign_bits, const void *e, int n_parties,
                                     lr_poly *const *shares);
int lr_setup_rkg_naive_key(lr_setup *s, const lr_poly *round2, lr_poly *evk_out);
int lr_setup_rtg_share(lr_setup *s, const lr_poly *sk, const uint64_t *galois_elements, int n_keys, const lr_poly *crp, const uint8_t *e,
                       lr_poly *const *shares);
int lr_setup_rtg_share_device(lr_setup *s, const lr_poly *sk, const uint64_t *galois_elements, int n_keys, const lr_poly *crp, const void *e,
                              lr_poly *const *shares);
int lr_setup_rtg_key(lr_setup *s, const lr_poly *share, const lr_poly *crp, lr_poly *rotkey_out);
int lr_setup_aggregate(lr_setup *s, const lr_poly *const *shares, int n_shares, lr_poly *out);

/* ------------------------------------------------------------------ multi-device ------ */
/* a batch of independent ciphertexts shards across the GPUs of a node by contiguous blocks (replicated contexts, tables
 * and keys, created per device with lr_context_create(..., device, ...)); nothing crosses devices but finished results.  The reference's
 * parallel model is goroutines in ONE process, one evaluator each (examples/dbfv/psi/psi.go:215-233): here one host thread per device,
 * every handle bound to its device, and these three entry points for the exchange -- no second process, no collective library.
 *
 * lr_poly_copy_peer: polys [src_index, src_index + count) of src -> slots [dst_index, ...) of dst (same N and limb count; any two devices
 * of the process, or the same one).  Asynchronous and ordered on the devices: the copy runs on a copy stream the library keeps per
 * (destination device, source device) pair -- xGMI is point-to-point, so the copies from different peers into one root use different links
 * at once -- behind an event recorded NOW on src_ctx's stream (it waits for everything enqueued through src_ctx before this call, e.g. the
 * kernels that produce the chunk), and overlaps whatever src_ctx is given next.  Nothing is enqueued on dst_ctx's stream: the consumer
 * calls lr_context_wait_peer_copies(dst_ctx) when it wants to read -- dst_ctx's stream then waits (on the device) for every copy into its
 * device enqueued so far.  Callable from any thread; the source must not be overwritten before the copy has run (the caller's ordering:
 * later work of src_ctx on those polys must follow an lr_context_wait_peer_copies / lr_context_sync of the consumer), and the destination
 * slots must not be in use by work still queued on dst_ctx when the call is made (the copy is not ordered behind dst_ctx's stream, so that a
 * root which computes its own share into other slots of the same poly keeps overlapping with the incoming copies).
 *
 * lr_gather_blocks: the whole gather in one call: block r = the first counts[r] polys of srcs[r], placed in dst one behind the other in
 * block order (= global unit order under contiguous-block sharding), then lr_context_wait_peer_copies(dst_ctx).  A producer that works in
 * chunks calls lr_poly_copy_peer per chunk instead and overlaps the copies with the next chunk's kernels (tools/multi_gpu_bench.cpp). */
int lr_poly_copy_peer(lr_context *dst_ctx, lr_poly *dst, int dst_index, lr_context *src_ctx, const lr_poly *src, int src_index, int count);
int lr_context_wait_peer_copies(lr_context *ctx);
int lr_gather_blocks(lr_context *dst_ctx, lr_poly *dst, lr_context *const *src_ctxs, const lr_poly *const *srcs, const int *counts, int n_blocks);

/* ------------------------------------------------------------------ measurement ------- */
/* HIP events on the context's stream (bench.py's roofline leg). */
int lr_timer_start(lr_context *ctx);
int lr_timer_stop(lr_context *ctx, float *elapsed_ms);   /* synchronises on the stop event */

#ifdef __cplusplus
}
#endif
#endif /* LATTIGO_RING_H */
