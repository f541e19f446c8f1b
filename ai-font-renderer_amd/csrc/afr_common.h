// afr_common.h -- shared device helpers and the internal launcher interface of libafr.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <type_traits>

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;

// ---------------------------------------------------------------------------------------------
// Dropout counter hash.  Bit-for-bit twin of ai-font-renderer_amd/synth.py:dropout_keep_mask.
// Stands in for the reference's torch bernoulli_ stream (model.py:137,144,149).
// ---------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint32_t afr_hash32(uint64_t idx, uint32_t key) {
    uint32_t lo = (uint32_t)idx, hi = (uint32_t)(idx >> 32);
    uint32_t h = lo * 0x9E3779B1u + (key + hi * 0x85EBCA6Bu);
    h ^= h >> 16; h *= 0x21F0AAADu;
    h ^= h >> 15; h *= 0x735A2D97u;
    h ^= h >> 15;
    return h;
}
// keep element idx iff the top 24 hash bits are below thr24 = keep_prob * 2^24
__host__ __device__ __forceinline__ bool afr_keep(uint64_t idx, uint32_t key, uint32_t thr24) {
    return (afr_hash32(idx, key) >> 8) < thr24;
}

static inline uint64_t afr_splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
enum { AFR_STREAM_EMBED = 1, AFR_STREAM_ATTN = 2, AFR_STREAM_FC = 3 };
static inline uint32_t afr_dropout_key(uint64_t seed, uint64_t step, uint64_t stream, uint64_t rank) {
    uint64_t v = seed ^ (step * 0x9E3779B97F4A7C15ull) ^ (stream * 0xC2B2AE3D27D4EB4Full) ^ (rank * 0x165667B19E3779F9ull);
    return (uint32_t)(afr_splitmix64(v) & 0xFFFFFFFFull);
}
static inline uint32_t afr_keep_threshold(float keep_prob) { return (uint32_t)((double)keep_prob * 16777216.0); }

// ---------------------------------------------------------------------------------------------
// wave64 reductions
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Block-level finish of a loss reduction: `block_sum` (valid in thread 0) is published as this block's partial; the
// LAST block to arrive sums all partials in block order (deterministic) and adds sum * inv_n to *loss_accum.
// Hand-off form: sc1 (write-through) partial store, drained, agent-scope ticket; the reader uses sc1 loads only
// (cdna_hip_programming.md Guideline 16 R1: no release fence -- it would flush every dirty line of the XCD's L2).
// Must be called by all threads of the block; `sh` is >= blockDim.x floats of LDS free for use.
// DEFERRABLE (the GEMM epilogues only): with counter == nullptr the block stores its partial -- the same sc1 store -- and
// returns: no ticket, no barrier, no last-block work.  A later launch of the same stream adds the partials with
// loss_sum_deferred (gemm.hip: the workgroup appended to glyph_l1_bwd_fused_kernel's grid).
template <bool DEFERRABLE = false>
__device__ __forceinline__ void loss_block_finish(float block_sum, float* partial, unsigned* counter, float* loss_accum,
                                                  float inv_n, float* sh) {
    __shared__ unsigned ticket_;
    if (DEFERRABLE && !counter) {
        if (threadIdx.x == 0) __hip_atomic_store(partial + blockIdx.x, block_sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(partial + blockIdx.x, block_sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ticket_ = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (ticket_ != gridDim.x - 1) return;
    float a = 0.f;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += blockDim.x)
        a += __hip_atomic_load(partial + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int o = blockDim.x >> 1; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss_accum[0] += sh[0] * inv_n;
        __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-arm for the next call
    }
}
// The partials that a launch of `n` blocks of `bd` threads left with counter == nullptr, added by ONE later workgroup of at least
// bd threads (all of them call): loss_block_finish's last-block arithmetic term for term -- the strided per-thread sums at the
// PRODUCER's block size, the same LDS tree, the same final expression -- so the loss is bit for bit the ticket form's.  The
// producer was an earlier launch of the same stream: plain loads.  The arrival counter is not touched (it stays zero).
struct LossSum {
    const float* partial = nullptr;   // NULL: nothing to add
    int n = 0, bd = 0;                // blocks and threads per block of the launch that wrote the partials
    float inv_n = 0.f;
    float* loss_accum = nullptr;
};
__device__ __forceinline__ void loss_sum_deferred(const LossSum& l, float* sh) {
    const int t = threadIdx.x, bd = l.bd;
    if (t < bd) {
        float a = 0.f;
        for (int i = t; i < l.n; i += bd) a += l.partial[i];
        sh[t] = a;
    }
    __syncthreads();
    for (int o = bd >> 1; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    if (t == 0) l.loss_accum[0] += sh[0] * l.inv_n;
}

// Loss kinds of a plan (afr_config.loss; the values of AFR_LOSS_* in afr.h).  The kind is a template parameter of every kernel
// that computes a loss or an output head: the LOSS_MSE instantiations hold no BCE code.
constexpr int LOSS_MSE = 0, LOSS_BCE = 1;
// The sigmoid head of a BCE plan, stable form: e = exp(-|u|) <= 1, so nothing overflows at either end.
__device__ __forceinline__ float sigmoid_of(float u, float e) {
    const float r = __builtin_amdgcn_rcpf(1.f + e);
    return u >= 0.f ? r : e * r;
}
__device__ __forceinline__ float sigmoid_f(float u) { return sigmoid_of(u, __expf(-fabsf(u))); }
// Binary cross-entropy on the logit u of ONE pixel with soft target t (F.binary_cross_entropy_with_logits): returns the loss
// term max(u,0) - t u + log1p(exp(-|u|)) and leaves du = (sigmoid(u) - t) * inv_n.  Every BCE site -- the loss kernel, the two
// GEMM epilogues, the fused small-net step -- calls this, so that fused and unfused paths give du bit for bit (sub then mul:
// nothing for the compiler to contract).  One v_exp_f32, one v_rcp_f32, one v_log_f32.  log1p is taken as log(1 + e): below
// e = 6e-8 the term is dropped, an absolute error per pixel smaller than one rounding of t u there; it saves the epilogues
// the registers and branches of a true log1p.
__device__ __forceinline__ float bce_logits_elem(float u, float t, float inv_n, float& du) {
    const float e = __expf(-fabsf(u));
    du = (sigmoid_of(u, e) - t) * inv_n;
    return fmaf(-t, u, fmaxf(u, 0.f)) + __logf(1.f + e);
}
// The loss head of ONE pixel: returns the loss term of u against target t and leaves du.  LOSS_MSE: (clamp(u,0,1) - t)^2 and
// du = 2 (clamp(u,0,1) - t) / mean_elems * [0<=u<=1] (reference model.py:156,268-270); g2 = 2 * inv_n is the caller's, hoisted out
// of its pixel loop (taken here it costs an instruction per pixel).  LOSS_BCE: bce_logits_elem.  Every loss site calls this.
template <int LOSS>
__device__ __forceinline__ float loss_elem(float u, float t, float inv_n, float g2, float& du) {
    if constexpr (LOSS == LOSS_BCE) return bce_logits_elem(u, t, inv_n, du);
    else {
        const float diff = fminf(fmaxf(u, 0.f), 1.f) - t;
        du = (u >= 0.f && u <= 1.f) ? g2 * diff : 0.f;
        return diff * diff;
    }
}
// 8 packed uint8 targets as floats, pixel / 255.0f (helpers.py:121): divided, or (LUT) looked up in the block's table of the 256
// quotients -- the same values.  (A kernel that has the table only sometimes branches at the call: one branch for the eight.)
template <bool LUT>
__device__ __forceinline__ void targets_u8x8(uint2 w, const float* lut255, float (&t)[8]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned a = (w.x >> (8 * r)) & 0xFF, b = (w.y >> (8 * r)) & 0xFF;
        t[r] = LUT ? lut255[a] : (float)a / 255.0f;
        t[4 + r] = LUT ? lut255[b] : (float)b / 255.0f;
    }
}
// What a loss site needs besides its logits.  One host function builds it (afr_api.hip loss_args).
struct LossArgs {
    const void* target = nullptr;   // [rows][cols] uint8 or float32; NULL in a GemmParams = no fused loss
    const int* rowmap = nullptr;    // optional: the targets of output row m are row rowmap[m] of target (a resident data set read in
                                    // place, 64-bit addressing); NULL = row m
    int tdtype = 0;                 // AFR_TARGET_*
    float inv_n = 0.f;              // 1 / mean_elems
    float* partial = nullptr;       // per-block partial sums (>= grid floats)
    unsigned* counter = nullptr;    // arrival counter, zero on entry, re-armed by the last block
    float* loss_accum = nullptr;    // device scalar: += sum(partials) / mean_elems
    int kind = LOSS_MSE;            // LOSS_MSE: clamp head + MSE; LOSS_BCE: sigmoid head + BCE with logits
};
// the target row of output row m (TROWS: an instantiation of its own, so that the dense kernels carry no row-map code)
template <bool TROWS> __device__ __forceinline__ int loss_target_row(const LossArgs& l, int m) { return TROWS ? l.rowmap[m] : m; }

// torch.optim.AdamW (reference model.py:273,310) with the step's scalars folded on the host (afr_api.hip adam_hyper):
//   p *= decay;  m += (g-m)*(1-b1);  v = b2*v + (1-b2)*g*g;  p -= step * m / (sqrt(v) * rsqrt_bc2 + eps)
struct AdamHyper { float decay = 1.f, b1 = 0.f, b2 = 0.f, eps = 0.f, step = 0.f /* lr / bc1 */, rsqrt_bc2 = 1.f; };
// The fused multiply-adds are spelled out: left to the compiler's contraction, one site (adamw_kernel, with its gradient scale
// ahead of the update) rounded b2 * v instead of (1 - b2) g g, and the data-parallel step no longer equalled the fused one bit
// for bit.  These are the forms every site of the parent compiled to.
__device__ __forceinline__ void adamw_elem(float& p, float& m, float& v, float g, const AdamHyper& h) {
    m = __builtin_fmaf(g - m, 1.f - h.b1, m);
    v = __builtin_fmaf(v, h.b2, (1.f - h.b2) * g * g);
    const float denom = __builtin_fmaf(sqrtf(v), h.rsqrt_bc2, h.eps);
    p = __builtin_fmaf(p, h.decay, -h.step * (m / denom));
}
// The same update as the f32 / bf16x3 tile epilogue has always computed it, one element at a time: the plain expressions, which
// the compiler does not fuse there.  Kept apart so that this path's weights stay what they were, bit for bit; it agrees with
// adamw_elem to the last bit only (tests/test_gpu_edges.py test_fused_optimizer_step_equals_unfused_step).
__device__ __forceinline__ void adamw_elem_plain(float& p, float& m, float& v, float g, const AdamHyper& h) {
    p *= h.decay;
    m = m + (g - m) * (1.f - h.b1);
    v = v * h.b2 + (1.f - h.b2) * g * g;
    const float denom = sqrtf(v) * h.rsqrt_bc2 + h.eps;
    p -= h.step * (m / denom);
}
// The update of four consecutive elements with gradient g; returns the new weights as the bf16 shadow's value.  A site loads
// and stores p/m/v(/shadow) its own way (streaming buffer loads, an LDS prefetch, nt stores, plain ones).
// (p/m/v as native vectors, updated element by element: repacked through float4 the 4-wave weight-gradient kernel allocated 247
// VGPRs for 206)
__device__ __forceinline__ bf16x4 adamw_quad(f32x4& p, f32x4& m, f32x4& v, f32x4 g, const AdamHyper& h) {
#pragma unroll
    for (int r = 0; r < 4; ++r) { float a = p[r], b = m[r], c = v[r]; adamw_elem(a, b, c, g[r], h); p[r] = a; m[r] = b; v[r] = c; }
    return (bf16x4){(bf16_t)p[0], (bf16_t)p[1], (bf16_t)p[2], (bf16_t)p[3]};
}

// Optimizer kinds of a plan (afr_set_optimizer; the values of AFR_OPT_* in afr.h).  Like the loss kind, a template parameter of
// every kernel that updates parameters: the OPT_ADAMW instantiations hold no Lion code and are the kernels they were.
constexpr int OPT_ADAMW = 0, OPT_LION = 1;
// Lion (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms"): one moment, the update is the sign of an interpolation.
//   c = b1*m + (1-b1)*g;  p = p*decay - lr*sign(c)  (sign(0) = 0);  m = b2*m + (1-b2)*g        decay = 1 - lr*wd
// Takes the AdamHyper of the step: decay, b1, b2 and step = lr (no bias correction: eps and rsqrt_bc2 are not read).  FMAs spelled
// out as in adamw_elem, and this is the ONLY statement of the update: given the same p, m, g every site agrees bit for bit.
__device__ __forceinline__ void lion_elem(float& p, float& m, float g, const AdamHyper& h) {
    const float c = __builtin_fmaf(g - m, 1.f - h.b1, m);
    const float s = (float)((c > 0.f) - (c < 0.f));
    p = __builtin_fmaf(p, h.decay, -h.step * s);
    m = __builtin_fmaf(g - m, 1.f - h.b2, m);
}
__device__ __forceinline__ bf16x4 lion_quad(f32x4& p, f32x4& m, f32x4 g, const AdamHyper& h) {
#pragma unroll
    for (int r = 0; r < 4; ++r) { float a = p[r], b = m[r]; lion_elem(a, b, g[r], h); p[r] = a; m[r] = b; }
    return (bf16x4){(bf16_t)p[0], (bf16_t)p[1], (bf16_t)p[2], (bf16_t)p[3]};
}
// The update of four elements by the kernel's optimizer kind (OPT_LION: v is neither read nor written)
template <int OPT>
__device__ __forceinline__ bf16x4 opt_quad(f32x4& p, f32x4& m, f32x4& v, f32x4 g, const AdamHyper& h) {
    if constexpr (OPT == OPT_LION) return lion_quad(p, m, g, h);
    else return adamw_quad(p, m, v, g, h);
}

// Runtime value -> template argument: f is a generic lambda and receives the value as a tag, `[&](auto rows) { k<rows()> ... }` or
// `[&](auto t) { using T = typename decltype(t)::type; ... }`.  Nest them; instantiate only what exists.
template <class T> struct TypeTag { using type = T; };
template <class F> static inline auto with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <class F> static inline auto with_loss(int kind, F&& f) {
    return kind == LOSS_BCE ? f(std::integral_constant<int, LOSS_BCE>{}) : f(std::integral_constant<int, LOSS_MSE>{});
}
template <class F> static inline auto with_opt(int kind, F&& f) {
    return kind == OPT_LION ? f(std::integral_constant<int, OPT_LION>{}) : f(std::integral_constant<int, OPT_ADAMW>{});
}
template <class F> static inline auto with_act(bool is_bf16, F&& f) { return is_bf16 ? f(TypeTag<bf16_t>{}) : f(TypeTag<float>{}); }

__device__ __forceinline__ float bf16_to_f32(bf16_t x) { return (float)x; }
__device__ __forceinline__ bf16_t f32_to_bf16(float x) { return (bf16_t)x; }

// ---------------------------------------------------------------------------------------------
// internal launchers (implemented in the .hip files, called from afr_api.cpp)
// ---------------------------------------------------------------------------------------------
// internal bit of GemmParams::flags (above the public AFR_GEMM_* bits of include/afr.h; set by the chained launcher only): the bf16
// output tile of a product on the 256x256 body is stored write-through (sc1), for readers inside the same launch
constexpr int AFR_GEMM_OUT_WTHRU = 1 << 20;
struct GemmParams {
    const void* A; const void* B; void* C; const float* bias; const void* aux;
    int M, N, K;
    int lda, ldb, ldc, ldaux;
    int flags;            // AFR_GEMM_* bits
    int splitk;           // >=1
    long long slab_stride;  // elements between split-K slabs of C
    // optional fused bias gradient (A must be k-strided): colsum[z*colsum_stride + m] = sum_k A(m,k) over split z
    float* colsum = nullptr;
    long long colsum_stride = 0;
    // optional fused loss (last forward layer of a training step; loss.target set): instead of u = A.B^T + bias the epilogue
    // writes du and accumulates the loss (loss_elem)
    LossArgs loss;
    // optional fused optimizer (dW GEMMs only, single GPU): C is the weight's gradient tile; instead of storing it
    // the epilogue applies AdamW to the matching tile of p/m/v (same [M][ldc] layout) and refreshes the bf16 shadow
    float* ad_p = nullptr; float* ad_m = nullptr; float* ad_v = nullptr; bf16_t* ad_shadow = nullptr;
    AdamHyper ad;
    // optional in-launch split-K (bf16, 256x256 tiles; gemm.hip gemm_bf16_256_body): the first head_tiles tiles of the
    // walk are computed whole, each remaining tile as `splitk` K-slices parked in fix_ws (256 KiB per slice) and summed in
    // slice order by the slice block that arrives last (fix_cnt: one zeroed counter per tail tile, re-armed by the kernel).
    // The output then takes the full epilogue (bias / ReLU / mask / bf16), unlike plain split-K's f32 partial slabs.
    int head_tiles = 0;
    int ad_kind = OPT_ADAMW;   // the fused optimizer's kind (OPT_*), read by the launchers only: it selects the instantiation.  (Declared
                               // here it takes the padding ahead of fix_ws: no kernel argument of the AdamW kernels moves.)
    float* fix_ws = nullptr; unsigned* fix_cnt = nullptr;
    // optional COOPERATIVE split-K (bf16, 256x256 tiles, grouped launches; gemm.hip gemm_bf16_256_body): the `splitk` (2, 4 or
    // 8) slice workgroups of a tile park their accumulators in coop_ws (256 KiB per slice, write-through), arrive on the
    // tile's counter and WAIT for each other (every workgroup of the launch is resident: one per CU); then slice z adds rows
    // [z, z+1) * 128 / splitk ... of every wave's accumulator image over all slices, in slice order, and finishes that strip:
    // AdamW on p/m/v (ad_p set) or a plain store into C.  No partial slabs leave the kernel and no second kernel re-reads
    // them.  coop_cnt: one counter per tile, monotonic: a launch waits for coop_target = launches so far * splitk.
    float* coop_ws = nullptr; unsigned* coop_cnt = nullptr; unsigned coop_target = 0; uint32_t* err = nullptr;
    // optional row gather (bf16): memory row r of the operand (a row m of a k-contiguous A, a row k of a k-strided B, a row m
    // of aux) is row rowmap[r] of the table the operand pointer names.  The glyph nets' first-layer output as a combination
    // table (elementwise.hip glyph_combo_kernel).  Supported: A k-contiguous on the 256x128 ring kernel, B k-strided on the
    // 256x256 kernel, aux with a bf16 output; the launchers refuse anything else.
    const int* a_rowmap = nullptr; const int* b_rowmap = nullptr; const int* aux_rowmap = nullptr;
    float out_scale = 1.f;     // fp8 products: scale_a * scale_b, applied to the accumulators ahead of bias / ReLU
    // optional ReLU mask as BITS (bf16 output only; N a multiple of 8): a forward layer with AFR_GEMM_RELU leaves bit (n & 7)
    // of mask_out[m * ldmask + n / 8] = [stored activation (m, n) > 0]; an input-gradient product with AFR_GEMM_RELU_MASK
    // reads mask_in in that layout INSTEAD of the activation aux (1/16 of its bytes: C3's 16.8 MB mask read becomes 1 MB)
    unsigned char* mask_out = nullptr; const unsigned char* mask_in = nullptr; int ldmask = 0;
    // AFR_GEMM_OUT_WTHRU (a chained launch's dX_up, set by its launcher): the arrival counters of the output's 256-row blocks
    unsigned* hand_cnt = nullptr;
#ifdef AFR_GEMM_TIMING
    int dbg_slot = 0;     // kernel-development builds: which 1024-block region of the stamp buffer this launch writes
#endif
};
constexpr uint32_t AFR_ERR_INDEX = 1u, AFR_ERR_COOP_TIMEOUT = 2u, AFR_ERR_ROW = 4u, AFR_ERR_GRAD_NONFINITE = 8u;    // bits of the plan's device error word
hipError_t afr_launch_gemm(int dtype, const GemmParams& p, hipStream_t s);
void afr_gemm_tile_launch_shape(int dtype, const GemmParams& p, int* tiles, int* threads);   // of a product on the ring / tile kernels
hipError_t afr_launch_gemm_fp8(const GemmParams& p, hipStream_t s);          // e4m3 x e4m3, both k-contiguous (gemm.hip fp8k)
hipError_t afr_launch_f32_to_fp8(const float* src, unsigned char* dst, long long n, float scale, hipStream_t s);
// several independent products in one launch (falls back to one launch each when one of them does not qualify)
bool afr_gemm_groupable(int dtype, const GemmParams& p);
hipError_t afr_launch_gemm_group(int dtype, const GemmParams* ps, int n, int tile256, hipStream_t s);
void afr_gemm_pair_plan(int B, int n_out, int k_in, int* tile256, int* splitk);
// two layers' cooperative 256x256 pairs as ONE chained launch (gemm.hip, GemmGroup::chain).  ps[4] in chain order: dW_up, dX_up,
// dW_lo, dX_lo, where dX_up's output is the dy of both lower products.  _counts: what the shapes allow on a device of `cus` CUs
// (host-only); _ok: these descriptors on the current device; _block: the kernel's block map (host copy).
bool afr_gemm_chain_counts(int B, int N_up, int K_up, int sk_up, int K_lo, int sk_lo, int cus, int* front, int* back);
bool afr_gemm_chain_ok(int dtype, const GemmParams* ps);
unsigned afr_gemm_chain_arrivals(const GemmParams* ps);
// The folded first layer's fused backward as a FIFTH role of the chained launch (gemm.hip GemmGroup::l1): the arguments of
// afr_launch_glyph_l1_bwd_fused, whose d1 must be dX_lo's output (ps[3].C, same leading dimension), and a second set of monotonic
// arrival counters, one per 256-row block of d1: every launch adds ceil(N1 / 256) arrivals to each (afr_gemm_chain_l1_arrivals)
// and its first-layer workgroups wait for `target`, the total after it.
struct ChainL1 {
    const void* d1 = nullptr; int ldd = 0; const void* h0 = nullptr; int ldh = 0; const void* W1T = nullptr;
    const int64_t* x = nullptr; const int64_t* font = nullptr; int B = 0, N1 = 0, vocab = 0, n_fonts = 0;
    float* slabs = nullptr; const int* h0_rowmap = nullptr; const LossSum* loss = nullptr;
    unsigned* cnt = nullptr; unsigned target = 0;
};
bool afr_gemm_chain_l1_ok(int dtype, const GemmParams* ps, const ChainL1& l1);       // afr_gemm_chain_ok and the role's own conditions
unsigned afr_gemm_chain_l1_arrivals(const GemmParams* ps);
hipError_t afr_launch_gemm_chain(int dtype, const GemmParams* ps, unsigned* hand_cnt, unsigned hand_target, uint32_t* err, hipStream_t s,
                                 const ChainL1* l1 = nullptr);
bool afr_gemm_chain_block(const GemmParams* ps, int b, int* member, int* tm, int* tn, int* slice);
// host copy of the block map of the first-layer range: block b of it (0 = the launch's block blk0[4]) -> its 64-glyph row block,
// its column range and the 256-row block of d1 it waits for; *loss_sum = 1 (the rest -1): the appended loss-sum workgroup, which
// exists only with deferred loss partials (has_loss).  false: b is outside the range.
bool afr_gemm_chain_l1_block(int B, int N1, bool has_loss, int b, int* row_block, int* col_range, int* wait_block, int* loss_sum);
// in-launch split-K for one bf16 product on 256x256 tiles (GemmParams::fix_ws): the workspace needs
// (tiles - head_tiles) * splitk * AFR_FIX_SLICE_BYTES
constexpr size_t AFR_FIX_SLICE_BYTES = 256 * 256 * 4;
hipError_t afr_launch_gemm_fix(const GemmParams& p, hipStream_t s);
const char* afr_gemm_kernel_name(int dtype, const GemmParams& p);
bool afr_gemm_wide_ok(int M, int N, int K);      // a bf16 product of this shape (no split, no fused optimizer) runs on the 256x128 ring kernel

hipError_t afr_launch_reduce(float* dst, const float* slabs, int nslabs, long long slab_stride, long long n,
                             float scale, int accumulate, hipStream_t s);
// grouped reduction: every gradient tensor that was produced as partial slabs, in ONE launch
struct RSeg {
    float* dst; const float* src; long long stride; long long n4; int nslabs; int blk0; int nblk; int deep;
    // optional (with the fused optimizer): a TRANSPOSED bf16 copy of this [tN][tK] weight, shT[k][n], kept current too
    bf16_t* shT = nullptr; int tN = 0, tK = 0;
};
// every gradient tensor of the deepest glyph net (AFR_MAX_HIDDEN + 1 Linears: weight + bias each) plus the folded first
// layer's extra segments (compact dW1, embedding and font partials) fits; afr_api.hip static_asserts it
constexpr int AFR_RT_MAXSEG = 32;
constexpr int AFR_L1F_MAX_SPLIT = 4;   // column ranges per row block of the fused first-layer backward (2 segments each)
struct RTable {
    int nseg = 0; int nblocks = 0; int overflow = 0;
    // optional fused optimizer: the summed gradient is not stored; AdamW is applied to p/m/v at the same flat offset
    // (offset of seg.dst from `gbase`)
    int adam = 0; AdamHyper ad;
    const float* gbase; float* P; float* M; float* V; bf16_t* shadow;
    RSeg seg[AFR_RT_MAXSEG];
    int kind = OPT_ADAMW;      // the fused optimizer's kind (OPT_*; V is not touched on OPT_LION), read by the launcher only -- last, so
                               // that no kernel argument of the AdamW instantiation moves
};
// optimizer groups (afr_set_param_groups): the table with one AdamHyper per segment behind it.  A kernel argument of its own, taken by
// the GROUPS instantiations of the grouped reduce only, so that no argument of the others moves.
struct RTableG { RTable t; AdamHyper seg_ad[AFR_RT_MAXSEG]; };
static_assert(sizeof(RTableG) <= 4096, "the grouped reduce's table travels by value as a kernel argument");
void afr_rtable_add(RTable& t, float* dst, const float* src, int nslabs, long long stride, long long n);
// seg_ad (optional, t.adam only): t.nseg hypers, segment k is updated with seg_ad[k] instead of t.ad
hipError_t afr_launch_reduce_group(const RTable& t, hipStream_t s, const AdamHyper* seg_ad = nullptr);
const char* afr_reduce_group_kernel_name(const RTable& t, const AdamHyper* seg_ad);      // "reduce_group<OPT,GROUPS>" of that launch
// The flat optimizer update (elementwise.hip adamw_kernel / opt_groups_kernel): AdamW or Lion over n elements (a multiple of 4) of p, g, m, v
// (and the bf16 shadow, optional), one launch.
// lr and wd besides h: the kernel folds its decay = 1 - lr * wd on the device, as it always has; h.decay is not read.
// sumsq (device word, optional): clip by global gradient norm -- every lane derives coef = clip_coef(*sumsq, |grad_scale|, max_norm)
// and the gradient enters the update as g * fl32(grad_scale * coef); a non-finite *sumsq leaves p/m/v/shadow untouched.
// sumsq NULL: the unclipped kernel, bit for bit what it has always computed.
// kind OPT_LION: the Lion update by the same kernel (v is not touched and may be NULL); the kernel folds decay = fl(1 - fl(lr * wd)),
// uncontracted, which is what adam_hyper hands the other sites as h.decay.
// tab (optional) -- optimizer groups: a slice whose tensors carry their own lr / weight decay, by the range-aware kernel.  Range k covers
// the quads (4 elements) [end4[k-1], end4[k]) of the FLAT buffer (end4[-1] = 0) and is updated with lr[k], wd[k] and step[k] = the
// AdamHyper::step of (lr[k], t), all folded on the host; the kernel folds decay from lr[k], wd[k] as the plain one does from lr, wd, which
// it does not read, nor h.step.  The table travels by value as a kernel argument.  The slice starts at flat element `first` (p, g, m, v,
// shadow point THERE) and end4[n - 1] * 4 >= first + n elements.
constexpr int AFR_OPT_MAX_RANGES = 128;
struct OptRangeTab { int n = 0; unsigned end4[AFR_OPT_MAX_RANGES]; float lr[AFR_OPT_MAX_RANGES], wd[AFR_OPT_MAX_RANGES], step[AFR_OPT_MAX_RANGES]; };
static_assert(sizeof(OptRangeTab) <= 3072, "the range table travels by value as a kernel argument");
struct FlatOpt {
    float* p; const float* g; float* m; float* v; bf16_t* shadow;
    long long n, first; const OptRangeTab* tab;
    float lr, wd; AdamHyper h;
    float grad_scale; const float* sumsq; float max_norm;
    int kind;
};
hipError_t afr_launch_flat_opt(const FlatOpt& f, hipStream_t s);
// Weight EMA (elementwise.hip ema_kernel): e = fma(p - e, fl(1 - decay), e) over n elements (a multiple of 4); sumsq as above: NULL,
// or the device word whose non-finite value leaves e untouched.
hipError_t afr_launch_ema(float* e, const float* p, long long n, float decay, const float* sumsq, hipStream_t s);
// Global gradient norm (elementwise.hip grad_sumsq_kernel): *out = sum of g[i]^2 over the tensor elements -- the (offset, numel)
// segments of the table `segs` (at most 256), flat-buffer padding excluded -- that lie inside [lo, hi) of g; lo, hi multiples of 4.
// scratch: AFR_SUMSQ_SCRATCH_FLOATS floats, zero before the first launch and left zero (block partials + arrival counter, the loss
// scratch's convention).  stats (optional): stats[0] = |grad_scale| * sqrt(sum), stats[1] = clip_coef.  err (optional): a
// non-finite sum sets AFR_ERR_GRAD_NONFINITE.  Fixed summation order: bitwise reproducible.
struct SumsqSeg { long long off, numel; };
constexpr int AFR_SUMSQ_MAX_BLOCKS = 1024, AFR_SUMSQ_COUNTER = 1024, AFR_SUMSQ_SCRATCH_FLOATS = 1032;
hipError_t afr_launch_grad_sumsq(const float* g, const SumsqSeg* segs /* device */, const SumsqSeg* segs_host /* the same table */, int nseg,
                                 long long lo, long long hi, float* scratch, float* out, float* stats, float grad_scale, float max_norm,
                                 uint32_t* err, hipStream_t s);
// Per-tensor statistics (elementwise.hip tstats_partial_kernel + tstats_finish_kernel; include/afr.h afr_tensor_stats): one
// afr_tensor_stat per (offset, numel) segment of a, or of a - minus (minus NULL: none), the padding between segments never read.
// Launch 1: one block per chunk of AFR_TSTATS_CHUNK elements of ONE segment (max(1, ceil(numel / CHUNK)) blocks per segment), one
// 32-byte partial record per block into `partial`; launch 2: one wave per segment adds its partials in chunk order.  The segment
// table reaches the kernels either as a device array (segs_dev: the plan's) or by value, built from segs_host (segs_dev NULL).
// segs_host is always given: the host needs the block counts.  The callers (afr_api.hip) have checked pointers, alignment and the table.
constexpr int AFR_TSTATS_CHUNK = 32768, AFR_TSTATS_MAX_SEGS = 256;
struct afr_tensor_stat;
static inline long long afr_tstats_seg_blocks(long long numel) {
    const long long nb = (numel + AFR_TSTATS_CHUNK - 1) / AFR_TSTATS_CHUNK;
    return nb ? nb : 1;
}
hipError_t afr_launch_tensor_stats(const float* a, const float* minus, const SumsqSeg* segs_dev, const SumsqSeg* segs_host, int nseg,
                                   afr_tensor_stat* out, afr_tensor_stat* partial, hipStream_t s);
// loss: u (act dtype) [rows][cols] -> du in place or to `du`; per-block partial sums to scratch, then
// a 1-block finisher adds sum(scratch) to *loss_accum (deterministic order).
int afr_mse_blocks(long long rows, long long cols);
// l.partial: >= afr_mse_blocks floats
hipError_t afr_launch_mse_grad(int act_dtype, const void* u, void* du, long long rows, long long cols, const LossArgs& l, hipStream_t s);
// evaluation of saved pre-activations (elementwise.hip eval_rows_kernel): per-row loss, 8-bit error counts against the targets, u8 levels.
// target NULL: q only.  cols % 8 == 0; a row belongs to one wave or one workgroup, the grid is capped and loops over the rows.
constexpr int AFR_EVAL_MAX_BLOCKS = 2048;
int afr_eval_blocks(long long rows, long long cols);
hipError_t afr_launch_eval_rows(int act_dtype, int loss_kind, const void* u, const void* target, int tdtype, const int* rowmap, long long rows,
                                long long cols, float* loss_rows, uint32_t* stats, uint8_t* q, hipStream_t s);
// Batch rows of a resident data set (afr_*_rows): validates and clamps rows[b] (AFR_ERR_ROW), writes ridx[b] = the narrowed index
// the loss kernels' row maps read and, when sx is not NULL, stages x[rows[b]][0 .. Lc) into sx [B][Lc] and font[rows[b]] into sfont.
hipError_t afr_launch_dataset_rows(const int64_t* rows, int B, long long n_rows, const int64_t* x, const int64_t* font, int L, int Lc,
                                   int* ridx, int64_t* sx, int64_t* sfont, uint32_t* err_flag, hipStream_t s);
hipError_t afr_launch_f32_to_bf16(const float* src, bf16_t* dst, long long n, hipStream_t s);
// the device data set (dataset.hip): the LCG text source, one lane per sample, and the sheet composer over a glyph atlas, one
// workgroup per sheet in a capped grid.  The composer keeps the atlas's cells and a glyph range per line and 8-pixel column block in dynamic LDS
// (afr_compose_dynamic_lds) beside afr_compose_static_lds() bytes of its own; the caller holds the sum under AFR_COMPOSE_LDS_BUDGET (what a workgroup may ask for without opting in to more).
constexpr int CMP_MAX_LDX = 256, CMP_MAX_LINES = 16, AFR_COMPOSE_MAX_BLOCKS = 2048, AFR_COMPOSE_LDS_BUDGET = 65536;
struct ComposeArgs {
    const uint8_t* cells; const int32_t* adv64; const int16_t* kern64;      // afr_glyph_atlas
    int n_codes, cell_h, cell_w, origin_x, origin_y;
    int height, width, wrap_width64, n_lines, baseline[CMP_MAX_LINES];      // afr_sheet_geometry
    const int64_t* codes; int ldx; const int64_t* out_rows; long long n; uint8_t* out; uint32_t* err;
};
size_t afr_compose_static_lds();
size_t afr_compose_dynamic_lds(int n_codes, int cell_h, int cell_w, int n_lines, int width);
int afr_compose_blocks(long long n);
hipError_t afr_launch_dataset_text(long long first_seed, const int64_t* seed_rows, const int64_t* out_rows, long long n, int min_len, int max_len,
                                   int64_t* codes, int ldx, int32_t* len, hipStream_t s);
hipError_t afr_launch_compose_sheets(const ComposeArgs& a, hipStream_t s);
// the weighted text source (cum: device [94] inclusive cumulative weights of the codes 33..126) and the one-workgroup launch that builds
// its table from afr_op_sheet_char_errors' by-code counters (members: host, bit i = code 33 + i)
hipError_t afr_launch_dataset_text_w(long long first_seed, const int64_t* seed_rows, const int64_t* out_rows, long long n, int min_len,
                                     int max_len, const uint32_t* cum, int64_t* codes, int ldx, int32_t* len, uint32_t* err, hipStream_t s);
hipError_t afr_launch_text_weights(const unsigned long long* by_code, const uint32_t members[3], uint32_t floor_w, uint32_t gain, uint32_t* cum,
                                   uint32_t* w, hipStream_t s);
// the first-order Markov text source (cum2: device [95][94], one row of inclusive cumulative weights per context: row 0 at a word's
// start, row 1 + i after letter i), the scatter of afr_op_sheet_char_errors' per-position records into the table by (preceding
// character, character) (by_pair: device [95][94][4], added to) and the one-workgroup launch that builds cum2 from that table
hipError_t afr_launch_dataset_text_m(long long first_seed, const int64_t* seed_rows, const int64_t* out_rows, long long n, int min_len,
                                     int max_len, const uint32_t* cum2, int64_t* codes, int ldx, int32_t* len, uint32_t* err, hipStream_t s);
hipError_t afr_launch_pair_errors(const int64_t* codes, int ldx, const int64_t* code_rows, long long n, const uint32_t* per_pos,
                                  unsigned long long* by_pair, hipStream_t s);
hipError_t afr_launch_pair_weights(const unsigned long long* by_pair, const uint32_t members[3], uint32_t floor_w, uint32_t gain,
                                   uint32_t min_chars, uint32_t* cum2, uint32_t* w2, hipStream_t s);
// afr_op_sheet_char_errors: compose's arguments (c.out unused, c.out_rows = the rows of codes the samples read) beside the dense
// prediction and the two outputs.  LDS as compose's, plus the position records and one 64-bit counter set per code.
struct CharErrArgs {
    ComposeArgs c;
    const uint8_t* pred; uint32_t* per_pos; unsigned long long* by_code;
};
size_t afr_charerr_static_lds();
size_t afr_charerr_dynamic_lds(int n_codes, int cell_h, int cell_w, int n_lines, int width);
hipError_t afr_launch_sheet_char_errors(const CharErrArgs& a, hipStream_t s);
// afr_op_sheet_read_back: compose's arguments (c.out unused, c.out_rows = the rows of codes the samples read) beside the dense
// prediction, the candidates' 94-bit mask and the three outputs.  LDS as compose's, plus the position records, one staged window
// (cell_h * cell_w halfwords) per wave and a 94 x 96 table of 16-bit confusion counters.
struct ReadBackArgs {
    ComposeArgs c;
    const uint8_t* pred; uint32_t members[3]; uint8_t* read; uint32_t* score; unsigned long long* confusion;
};
size_t afr_readback_static_lds();
size_t afr_readback_dynamic_lds(int n_codes, int cell_h, int cell_w, int n_lines, int width);
hipError_t afr_launch_sheet_read_back(const ReadBackArgs& a, hipStream_t s);
// the output head and its backward for a caller-side loss: clamp(u, 0, 1), or sigmoid(u) on a LOSS_BCE plan
hipError_t afr_launch_clamp_bwd(int act_dtype, void* u_inout, const float* dy, long long n, hipStream_t s, int loss_kind = LOSS_MSE);
hipError_t afr_launch_clamp_out(int act_dtype, const void* u, float* y, long long n, hipStream_t s, int loss_kind = LOSS_MSE);
// glyph embedding gather / deterministic scatter-add
hipError_t afr_launch_glyph_embed(int act_dtype, const float* emb, const float* font_emb, const int64_t* x,
                                  const int64_t* font, int B, int E, int vocab, int n_fonts, void* out,
                                  uint32_t* err_flag, hipStream_t s);
// (the glyph getters below are also exported, include/afr.h: a caller of the afr_op_glyph_* entries sizes its buffers with them)
extern "C" int afr_embed_bwd_blocks(int B);
size_t afr_glyph_embed_bwd_lds_bytes(int E, int vocab, int n_fonts);      // dynamic LDS of glyph_embed_bwd_kernel; at most 160 KiB fit
hipError_t afr_launch_glyph_l1_fwd(int act_dtype, const float* emb, const float* font_emb, const float* W1, const float* b1,
                                   const int64_t* x, const int64_t* font, int B, int E, int N1, int vocab, int n_fonts,
                                   float* table, void* h0, void* h1, uint32_t* err_flag, hipStream_t s, void* w1t = nullptr);
hipError_t afr_launch_glyph_combo(const float* emb, const float* font_emb, const float* W1, const float* b1, const int64_t* x,
                                  const int64_t* font, int B, int E, int N1, int vocab, int n_fonts, float* table, void* h1c,
                                  int ld1 /* row stride of h1c, elements */, void* h0c, int* cidx, uint32_t* err_flag, hipStream_t s,
                                  void* w1t);
extern "C" int afr_glyph_k0(int E, int vocab, int n_fonts);
extern "C" int afr_glyph_l1_bwd_blocks(int N1);
// the same backward in one kernel (throughput mode, gemm.hip: glyph_l1_bwd_fused_kernel); W1T = bf16 [E][N1] from the forward
extern "C" int afr_glyph_l1_bwd_fused_eligible(int dtype, int E, int N1, int vocab, int n_fonts);   // 1 / 0
extern "C" int afr_glyph_l1_bwd_fused_split(int B, int N1);                       // column ranges per block of 64 glyphs
extern "C" int afr_glyph_l1_bwd_fused_blocks(int B, int N1);
extern "C" long long afr_glyph_l1_bwd_fused_slab_floats(int B, int N1, int vocab, int n_fonts);   // [dW1 nc*E | db1 nc | dTab rows*E], nc = N1 / split
hipError_t afr_launch_glyph_l1_bwd_fused(const void* d1, int ldd, const void* h0, int ldh, const void* W1T, const int64_t* x,
                                         const int64_t* font, int B, int N1, int vocab, int n_fonts, float* slabs, hipStream_t s,
                                         const int* h0_rowmap = nullptr, const LossSum* loss = nullptr);   // loss: one more workgroup adds deferred partials
hipError_t afr_launch_glyph_l1_bwd(const float* slabs, int nslabs, long long slab_stride, const float* W1, int N1, int E,
                                   int vocab, int n_fonts, float* dw1, float* dtab_part, hipStream_t s);
hipError_t afr_launch_glyph_embed_bwd(int act_dtype, const void* d, const int64_t* x, const int64_t* font, int B,
                                      int E, int vocab, int n_fonts, float* slabs /*[blocks][(vocab+n_fonts)*E]*/,
                                      hipStream_t s);

// sheet front end (sheet.hip)
struct SheetDims { int L, Lmax, E, H, F, vocab; };
constexpr int AFR_SHEET_SAVE_PER_POS = 56;   // 32 + 4 + 4 + 16, see SheetDrop::save
struct SheetParams {   // device pointers into the flat f32 parameter buffer
    const float *pos, *emb, *w_in, *b_in, *w_o, *b_o, *ln_g, *ln_b, *w1, *b1;
};
struct SheetDrop {
    uint32_t key_e, key_a, key_f, thr_e, thr_a, thr_f; float sc_e, sc_a, sc_f; int training;
    // optional per-string save area written by a training forward and read by backward: [B][L*AFR_SHEET_SAVE_PER_POS]
    // words = attention output o [L][32], softmax row max [4][L], 1/row-sum [4][L], and the attention-dropout keep bits
    // [4][L][4] (row (h,i), key j: bit (j>>1)&31 of word (j&1)*2 + (j>>6)).  Spares backward the attention recompute
    // and both of its passes the per-element counter hash (3 quarter-rate integer multiplies per probability).
    float* save;
    // optional inspection output (afr_debug_sheet_gather): the rows the kernel's embedding gather fetched, e0 [B][L][32] f32,
    // before dropout and positional encoding (model.py:167)
    float* dbg_e0 = nullptr;
};
// offsets (in floats) of the 10 small tensors inside one partial-gradient slab == their flat-buffer offsets
struct SheetSlabOff { int pos, emb, win, bin, wo, bo, g, b, w1, b1, total; };
extern "C" int afr_sheet_blocks(int B);   // (also exported, include/afr.h: a caller of the afr_op_sheet_* entries sizes its slabs with it)
size_t afr_sheet_fwd_lds_bytes(const SheetDims& d);
size_t afr_sheet_bwd_lds_bytes(const SheetDims& d);
hipError_t afr_launch_sheet_fwd(int act_dtype, const SheetDims& d, const SheetParams& P, const SheetDrop& dr,
                                const int64_t* x, int ldx, int B, void* z, float ln_eps, uint32_t* err_flag,
                                hipStream_t s);
hipError_t afr_launch_sheet_bwd(int act_dtype, const SheetDims& d, const SheetParams& P, const SheetDrop& dr,
                                const int64_t* x, int ldx, int B, const void* dz, float ln_eps, float* slabs,
                                const SheetSlabOff& so, hipStream_t s);

// fused step of the small one-hidden-layer glyph nets (glyph_fused.hip)
struct Glyph1Args {
    const int64_t* x; const int64_t* font;
    LossArgs loss;                           // targets [B][P] (rowmap: of glyph b = row rowmap[b]), the loss scratch and kind
    int B, E, N1, P, vocab, n_fonts;
    const float *emb, *femb, *b1, *b2;       // f32 masters
    const void *W1, *W2;                     // [N1][E], [P][N1] in the operand type (f32 masters / bf16 shadow)
    const void *W1T, *W2T;                   // bf16 mode: [E][N1], [N1][P]; f32 mode: the f32 masters again (gathered)
    float* slabs; long long slab_stride;     // slab b: this block's partial gradients, flat-buffer layout
    long long o_emb, o_font, o_w1, o_b1, o_w2, o_b2;
    uint32_t* err;
    int cs = 1;                              // column split: cs blocks share a row block, each owning P / cs output columns
};
// (rows, colsplit, blocks and eligible are also exported, include/afr.h: a caller of afr_op_glyph1_step sizes its buffers with them)
extern "C" int afr_glyph1_rows(int dtype);
extern "C" int afr_glyph1_colsplit(int dtype, int B, int P);     // blocks per row block (1, 2 or 4) for a batch of B
extern "C" int afr_glyph1_blocks(int dtype, int B, int P);       // row blocks x column split: the blocks (= slabs, loss partials) of a batch of B
int afr_glyph1_max_blocks(int dtype, int max_batch, int P);   // the most blocks any batch <= max_batch launches (slab / loss-partial count)
extern "C" int afr_glyph1_eligible(int E, int N1, int P, int vocab, int n_fonts);   // 1 / 0
size_t afr_glyph1_lds_bytes(int dtype, int E, int N1, int P, int table_rows);
hipError_t afr_launch_transpose_bf16(const float* W, bf16_t* WT, int N, int K, hipStream_t s);
hipError_t afr_launch_glyph1_step(int dtype, const Glyph1Args& a, hipStream_t s);

// per-pixel-token transformer (pixel.hip): the token-wise kernels of BASELINE configs[4], forward and backward
hipError_t afr_launch_pixel_ctx(int act_dtype, const float* emb, const float* femb, const int64_t* x, const int64_t* font, int B, int d,
                                int vocab, int n_fonts, void* ctx, uint32_t* err, hipStream_t s);
hipError_t afr_launch_pixel_add_ln(int act_dtype, const float* hin, float* h, const float* pos, const void* add, const float* g, const float* b, void* n,
                                   long long rows, int Tk, int d, float eps, hipStream_t s);
hipError_t afr_launch_pixel_attn(int act_dtype, const void* q, const void* kv, void* o, long long rows, int Tk, int d, int heads, int C, hipStream_t s);
hipError_t afr_launch_pixel_head(int act_dtype, const float* hin, float* h, const void* add, const float* g, const float* b, const float* w_out, const float* b_out,
                                 float* u, float* y, long long rows, int d, float eps, hipStream_t s, int loss_kind = LOSS_MSE);
// (these two are also exported, include/afr.h: a caller of the afr_op_pixel_* entries sizes its partial slabs with them)
extern "C" int afr_pixel_bwd_blocks(long long rows);    // blocks (= partial slabs) of the head / LayerNorm backward kernels
extern "C" int afr_pixel_attn_chunk(int Tk);            // tokens per attention-backward block
hipError_t afr_launch_pixel_head_bwd(int act_dtype, const float* du, const float* hf, const float* g, const float* b, const float* w_out, float* dh,
                                     void* dhT, float* part /*[blocks][4][d]: dgamma, dbeta, dw_out, db_out*/, long long rows, int d, float eps, hipStream_t s);
hipError_t afr_launch_pixel_ln_bwd(int act_dtype, const void* dy, const float* hin, const float* g, float* dh, void* dhT, float* part /*[blocks][2][d]*/,
                                   long long rows, int d, float eps, hipStream_t s);
hipError_t afr_launch_pixel_attn_bwd(int act_dtype, const void* dO, const void* q, const void* kv, void* dq, float* dkv_part /*[chunks][B][2][2d]*/,
                                     int B, int Tk, int d, int C, hipStream_t s);
hipError_t afr_launch_pixel_ctx_bwd(const float* dctx, const int64_t* x, const int64_t* font, int B, int d, int vocab, int n_fonts, float* demb, float* dfont,
                                    hipStream_t s);
hipError_t afr_launch_pixel_accum(int act_dtype, float* acc, const void* src, long long n, int first, hipStream_t s);
hipError_t afr_launch_pixel_cast(int act_dtype, void* dst, const float* src, long long rows, int w, int ld_src, hipStream_t s);
