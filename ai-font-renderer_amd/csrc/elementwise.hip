// elementwise.hip -- the HBM-bound kernels of the hot path: loss/grad reduction, AdamW, slab reduction,
// the glyph embedding gather and its deterministic scatter-add (bias gradients are fused into the dW GEMM).
// All are 16-byte-per-lane streaming kernels with grid-stride loops; reductions are shuffle -> LDS ->
// per-block partial -> fixed-order finish, so every result is bitwise reproducible run to run.
#include <algorithm>
#include "afr_common.h"
#include "../../include/afr.h"

int afr_glyph_k0(int E, int vocab, int n_fonts);
static inline int grid_for(long long work_items, int block, int max_blocks = 2048) {
    long long g = (work_items + block - 1) / block;
    if (g < 1) g = 1;
    if (g > max_blocks) g = max_blocks;
    return (int)g;
}

// ------------------------------------------------------------------------------------- reduce
// dst[i] = (accumulate ? dst[i] : 0) + scale * sum_s slabs[s*stride + i]   (fixed s order)
__global__ __launch_bounds__(256) void reduce_slabs_kernel(float* __restrict__ dst, const float* __restrict__ slabs,
                                                           int nslabs, long long stride, long long n, float scale,
                                                           int accumulate) {
    const long long n4 = n >> 2;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int s = 0; s < nslabs; ++s) {
            const float4 v = *reinterpret_cast<const float4*>(slabs + s * stride + 4 * i);
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
        a.x *= scale; a.y *= scale; a.z *= scale; a.w *= scale;
        float4* d = reinterpret_cast<float4*>(dst) + i;
        if (accumulate) { float4 o = *d; a.x += o.x; a.y += o.y; a.z += o.z; a.w += o.w; }
        *d = a;
    }
    // tail (n not a multiple of 4)
    for (long long i = (n4 << 2) + blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float a = 0.f;
        for (int s = 0; s < nslabs; ++s) a += slabs[s * stride + i];
        a *= scale;
        if (accumulate) a += dst[i];
        dst[i] = a;
    }
}
hipError_t afr_launch_reduce(float* dst, const float* slabs, int nslabs, long long slab_stride, long long n,
                             float scale, int accumulate, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, s, dst, slabs, nslabs,
                       slab_stride, n, scale, accumulate);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ grouped reduce
// (Optionally fused with AdamW: single-GPU steps update p/m/v right here and never materialise those gradients.)
// One launch sums every slab-produced gradient of a backward pass (split-K dW slabs, fused bias partials, embedding
// partials) into the flat gradient buffer, each in fixed slab order.  Block -> segment by a scan of <= 24 entries.
// sum of slabs [s0, s1) of one float4 column, 8 independent 16-byte loads in flight, fixed order
__device__ __forceinline__ float4 slab_sum(const float* src, long long stride, int s0, int s1) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    int s = s0;
    for (; s + 8 <= s1; s += 8) {
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(src + (long long)(s + u) * stride);
#pragma unroll
        for (int u = 0; u < 8; ++u) { a.x += v[u].x; a.y += v[u].y; a.z += v[u].z; a.w += v[u].w; }
    }
#pragma unroll 4
    for (; s < s1; ++s) {
        const float4 v = *reinterpret_cast<const float4*>(src + (long long)s * stride);
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    return a;
}
template <int OPT>
__device__ __forceinline__ void reduce_finish(const RTable& t, const AdamHyper& ad, const RSeg& sg, long long i, float4 a, f32x4 pp, f32x4 mm, f32x4 vv) {
    if (t.adam) {
        const long long off = (sg.dst - t.gbase) + 4 * i;
        const bf16x4 o = opt_quad<OPT>(pp, mm, vv, (f32x4){a.x, a.y, a.z, a.w}, ad);
        *reinterpret_cast<f32x4*>(t.P + off) = pp;
        *reinterpret_cast<f32x4*>(t.M + off) = mm;
        if constexpr (OPT == OPT_ADAMW) *reinterpret_cast<f32x4*>(t.V + off) = vv;
        if (t.shadow) *reinterpret_cast<bf16x4*>(t.shadow + off) = o;
        if (sg.shT) {                      // 4 consecutive k of one row n (tK is a multiple of 4)
            const int n = (int)((4 * i) / sg.tK), k = (int)(4 * i - (long long)n * sg.tK);
#pragma unroll
            for (int r = 0; r < 4; ++r) sg.shT[(size_t)(k + r) * sg.tN + n] = (bf16_t)pp[r];
        }
    } else {
        reinterpret_cast<float4*>(sg.dst)[i] = a;
    }
}
// OPT: the optimizer kind of a fused step (t.adam); the OPT_LION instantiation neither loads nor stores V
// GROUPS (optimizer groups, afr_set_param_groups): the argument is an RTableG and the block's segment is updated with ITS hyper
// (seg_ad[si], looked up by the host from the segment's flat offset) instead of the table's one; with GROUPS false the body is as it was.
__device__ __forceinline__ const RTable& rtable_of(const RTable& t) { return t; }
__device__ __forceinline__ const RTable& rtable_of(const RTableG& t) { return t.t; }
__device__ __forceinline__ const AdamHyper& hyper_of(const RTable& t, int) { return t.ad; }
__device__ __forceinline__ const AdamHyper& hyper_of(const RTableG& t, int si) { return t.seg_ad[si]; }
template <int OPT = OPT_ADAMW, bool GROUPS = false>
__global__ __launch_bounds__(256) void reduce_group_kernel(std::conditional_t<GROUPS, RTableG, RTable> tt) {
    const RTable& t = rtable_of(tt);
    int si = 0;
    for (int k = 1; k < t.nseg; ++k) if ((int)blockIdx.x >= t.seg[k].blk0) si = k;
    const RSeg sg = t.seg[si];
    const AdamHyper& ad = hyper_of(tt, si);
    f32x4 pp = {0.f, 0.f, 0.f, 0.f}, mm = pp, vv = pp;
    if (sg.deep) {
        // many slabs, few columns (the per-block partials of the sheet backward): a block owns 64 float4 columns and
        // each of its 4 waves sums a quarter of the slabs; the quarters meet in LDS and are added in wave order.
        __shared__ float4 part[3][64];
        const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
        const int per = (sg.nslabs + 3) >> 2;
        for (long long i0 = (long long)(blockIdx.x - sg.blk0) * 64; i0 < sg.n4; i0 += (long long)sg.nblk * 64) {
            const long long i = i0 + col;
            const bool live = i < sg.n4;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live) {
                if (grp == 0 && t.adam) {
                    const long long off = (sg.dst - t.gbase) + 4 * i;
                    pp = *reinterpret_cast<f32x4*>(t.P + off); mm = *reinterpret_cast<f32x4*>(t.M + off);
                    if constexpr (OPT == OPT_ADAMW) vv = *reinterpret_cast<f32x4*>(t.V + off);
                }
                const int s0 = grp * per, s1 = min(sg.nslabs, s0 + per);
                a = slab_sum(sg.src + 4 * i, sg.stride, s0, s1);
            }
            if (grp) part[grp - 1][col] = a;
            __syncthreads();
            if (grp == 0 && live) {
#pragma unroll
                for (int g = 0; g < 3; ++g) { const float4 v = part[g][col]; a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
                reduce_finish<OPT>(t, ad, sg, i, a, pp, mm, vv);
            }
            __syncthreads();
        }
        return;
    }
    for (long long i = (long long)(blockIdx.x - sg.blk0) * 256 + threadIdx.x; i < sg.n4; i += (long long)sg.nblk * 256) {
        if (t.adam) {   // issued ahead of the slab loads so that everything this element needs is in flight at once
            const long long off = (sg.dst - t.gbase) + 4 * i;
            pp = *reinterpret_cast<f32x4*>(t.P + off); mm = *reinterpret_cast<f32x4*>(t.M + off);
            if constexpr (OPT == OPT_ADAMW) vv = *reinterpret_cast<f32x4*>(t.V + off);
        }
        const float4 a = slab_sum(sg.src + 4 * i, sg.stride, 0, sg.nslabs);
        reduce_finish<OPT>(t, ad, sg, i, a, pp, mm, vv);
    }
}
void afr_rtable_add(RTable& t, float* dst, const float* src, int nslabs, long long stride, long long n) {
    if (n <= 0) return;
    if (t.nseg >= AFR_RT_MAXSEG) { t.overflow = 1; return; }     // the launch refuses an overflowed table: never a silent drop
    RSeg& sg = t.seg[t.nseg];
    sg.dst = dst; sg.src = src; sg.stride = stride; sg.n4 = n / 4; sg.nslabs = nslabs; sg.blk0 = t.nblocks;
    sg.shT = nullptr; sg.tN = sg.tK = 0;
    sg.deep = nslabs >= 32;
    const int cols = sg.deep ? 64 : 256;
    long long nb = (sg.n4 + cols - 1) / cols;       // one float4 per thread where possible: measured 2x faster than
    if (nb > 1024) nb = 1024;                       // 4 per thread (the kernel lives on memory-level parallelism)
    sg.nblk = (int)nb;
    t.nblocks += (int)nb;
    t.nseg++;
}
hipError_t afr_launch_reduce_group(const RTable& t, hipStream_t s, const AdamHyper* seg_ad) {
    if (t.overflow || (seg_ad && !t.adam)) return hipErrorInvalidValue;
    if (t.nseg == 0) return hipSuccess;
    if (seg_ad) {
        RTableG tg;
        tg.t = t;
        for (int k = 0; k < t.nseg; ++k) tg.seg_ad[k] = seg_ad[k];
        with_opt(t.kind, [&](auto opt) { hipLaunchKernelGGL((reduce_group_kernel<opt(), true>), dim3(t.nblocks), dim3(256), 0, s, tg); });
        return hipGetLastError();
    }
    with_opt(t.adam ? t.kind : OPT_ADAMW, [&](auto opt) { hipLaunchKernelGGL(reduce_group_kernel<opt()>, dim3(t.nblocks), dim3(256), 0, s, t); });
    return hipGetLastError();
}
// the instantiation afr_launch_reduce_group takes for (t, seg_ad), as <OPT,GROUPS>: the launcher's own two decisions, restated beside it
const char* afr_reduce_group_kernel_name(const RTable& t, const AdamHyper* seg_ad) {
    const bool lion = t.adam && t.kind == OPT_LION;
    return seg_ad ? (lion ? "reduce_group<1,1>" : "reduce_group<0,1>") : (lion ? "reduce_group<1,0>" : "reduce_group<0,0>");
}

// -------------------------------------------------------------------------------------- AdamW
// torch.optim.AdamW single-tensor update (reference model.py:273,310), one pass over p,g,m,v:
//   p *= 1 - lr*wd;  m += (g-m)*(1-b1);  v = b2*v + (1-b2)*g*g;  p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
// Also refreshes the bf16 shadow copy the bf16 GEMMs read.  28 (+2) bytes per element of HBM traffic.
// CLIP (clipping by global gradient norm, afr_set_grad_clip): every lane loads the one word *sumsq and derives the coefficient
// itself (clip_coef: the same few instructions everywhere, so every slice and every rank agrees); the gradient enters the update
// as g * fl32(gscale * coef) -- one rounded factor, then one rounded product that is NOT contracted into adamw_quad's FMAs
// (mul_rn).  A non-finite *sumsq skips the step: nothing is written.  The CLIP = false instantiation is the kernel as it was.
// OPT_LION (afr_set_optimizer): the same walk with lion_quad on p, g, m -- v is neither loaded nor stored, 20 (+2) bytes per element;
// step_size carries lr.  Its scalars are folded without contraction, clipped or not: decay = fl(1 - fl(lr * wd)) as the host hands it
// to the fused sites, and the gradient enters as fl(g * gscale), so that every Lion site sees the same decay and the same g.
__device__ __forceinline__ float clip_coef(float sumsq, float gscale_abs, float max_norm, float& total_norm) {
    total_norm = gscale_abs * sqrtf(sumsq);
    return fminf(1.f, max_norm / (total_norm + 1e-6f));      // torch.nn.utils.clip_grad_norm_, in f32
}
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.402823466e38f; }
// The pieces of the flat update, stated once for its two walks (adamw_kernel, opt_groups_kernel): what they share cannot drift apart.
// The clip prologue: false = a non-finite *sumsq, the block returns and nothing is written.
template <bool CLIP>
__device__ __forceinline__ bool flat_clip(float& gscale, const float* __restrict__ sumsq, float max_norm) {
    if constexpr (CLIP) {
        const float ss = *sumsq;
        if (!finite_f(ss)) return false;
        float tn;
        gscale = mul_rn(gscale, clip_coef(ss, fabsf(gscale), max_norm, tn));
    }
    return true;
}
// the decay of one (lr, wd), per launch or per range
template <int OPT> __device__ __forceinline__ float flat_decay(float lr, float wd) { return OPT == OPT_LION ? 1.f - mul_rn(lr, wd) : 1.f - lr * wd; }
// one quad of p, g, m(, v) in flight: loaded, then updated with h and stored (v and the shadow where the kind / the caller has them)
template <int OPT>
struct FlatQuad {
    float4 p4, gg, m4, v4;
    __device__ __forceinline__ void load(const float* __restrict__ p, const float* __restrict__ g, const float* __restrict__ m, const float* __restrict__ v,
                                         long long i) {
        p4 = reinterpret_cast<const float4*>(p)[i];
        gg = reinterpret_cast<const float4*>(g)[i];
        m4 = reinterpret_cast<const float4*>(m)[i];
        if constexpr (OPT == OPT_ADAMW) v4 = reinterpret_cast<const float4*>(v)[i];
    }
    template <bool CLIP>
    __device__ __forceinline__ void step(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, bf16_t* __restrict__ shadow, long long i,
                                         float gscale, const AdamHyper& h) const {
        f32x4 pp = {p4.x, p4.y, p4.z, p4.w}, mm = {m4.x, m4.y, m4.z, m4.w}, vv = {v4.x, v4.y, v4.z, v4.w};
        const f32x4 ge = (CLIP || OPT == OPT_LION) ? (f32x4){mul_rn(gg.x, gscale), mul_rn(gg.y, gscale), mul_rn(gg.z, gscale), mul_rn(gg.w, gscale)}
                                                   : (f32x4){gg.x * gscale, gg.y * gscale, gg.z * gscale, gg.w * gscale};
        const bf16x4 o = opt_quad<OPT>(pp, mm, vv, ge, h);
        reinterpret_cast<float4*>(p)[i] = make_float4(pp[0], pp[1], pp[2], pp[3]);
        reinterpret_cast<float4*>(m)[i] = make_float4(mm[0], mm[1], mm[2], mm[3]);
        if constexpr (OPT == OPT_ADAMW) reinterpret_cast<float4*>(v)[i] = make_float4(vv[0], vv[1], vv[2], vv[3]);
        if (shadow) reinterpret_cast<bf16x4*>(shadow)[i] = o;
    }
};
template <bool CLIP, int OPT = OPT_ADAMW>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v,
                                                    bf16_t* __restrict__ shadow, long long n4, float lr, float b1,
                                                    float b2, float eps, float wd, float step_size, float rsqrt_bc2,
                                                    float gscale, const float* __restrict__ sumsq, float max_norm) {
    const AdamHyper h{flat_decay<OPT>(lr, wd), b1, b2, eps, step_size, rsqrt_bc2};
    if (!flat_clip<CLIP>(gscale, sumsq, max_norm)) return;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        FlatQuad<OPT> q{};
        q.load(p, g, m, v, i);
        q.template step<CLIP>(p, m, v, shadow, i, gscale, h);
    }
}

// ----------------------------------------------------------------------------- optimizer groups
// adamw_kernel's walk over a slice whose tensors carry their own (lr, wd): afr_set_param_groups / afr_op_opt_groups.  ONE launch for the
// whole slice, the grid adamw_kernel would take.  The range table arrives by value; the block's first tab.n lanes fold each range's
// decay with the function adamw_kernel folds it with from its scalars (so a range is updated bit for bit as adamw_kernel<CLIP, OPT> would
// update it with that range's lr, wd) and park (end, decay, step) in LDS, ends relative to the slice.  A lane keeps a cursor into the table that
// only moves forward as its grid-stride index grows: at most tab.n LDS reads over the lane's whole life on top of two per quad, and no
// extra global traffic -- the 16-byte accesses and the 28 (+2) / 20 (+2) bytes per element are adamw_kernel's.  Lanes of one wave may sit
// in different ranges (tensor offsets are multiples of 64 elements, a wave covers 256).  No pow, no division: step is the host's.
template <bool CLIP, int OPT>
__global__ __launch_bounds__(256) void opt_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, bf16_t* __restrict__ shadow, long long n4, unsigned first4,
                                                         float b1, float b2, float eps, float rsqrt_bc2, float gscale,
                                                         const float* __restrict__ sumsq, float max_norm, OptRangeTab tab) {
    __shared__ unsigned s_end[AFR_OPT_MAX_RANGES];
    __shared__ float s_decay[AFR_OPT_MAX_RANGES], s_step[AFR_OPT_MAX_RANGES];
    if (!flat_clip<CLIP>(gscale, sumsq, max_norm)) return;
    // the first trip's loads are issued AHEAD of the table staging, so that the block's start-up (table loads, LDS, barrier) hides
    // behind them instead of standing in front of its first byte in flight
    const long long stride = (long long)gridDim.x * 256;
    long long i = blockIdx.x * 256ll + threadIdx.x;
    FlatQuad<OPT> q{};
    if (i < n4) q.load(p, g, m, v, i);
    if ((int)threadIdx.x < tab.n) {
        const int k = threadIdx.x;
        const float lr = tab.lr[k], wd = tab.wd[k];      // (read ahead of end4: the other order costs a scalar instruction)
        const unsigned e = tab.end4[k];
        s_end[k] = e > first4 ? e - first4 : 0u;
        s_decay[k] = flat_decay<OPT>(lr, wd);
        s_step[k] = tab.step[k];
    }
    __syncthreads();
    const int last = tab.n - 1;
    int cur = 0;
    while (i < n4) {
        while (cur < last && (unsigned long long)i >= s_end[cur]) ++cur;      // (the last range reaches the end of the slice)
        q.template step<CLIP>(p, m, v, shadow, i, gscale, AdamHyper{s_decay[cur], b1, b2, eps, s_step[cur], rsqrt_bc2});
        i += stride;
        if (i < n4) q.load(p, g, m, v, i);
    }
}
// f.tab == nullptr: adamw_kernel over the n elements with (f.lr, f.wd); else opt_groups_kernel with the table's ranges
hipError_t afr_launch_flat_opt(const FlatOpt& f, hipStream_t s) {
    if (f.n <= 0) return hipSuccess;
    if (f.n & 3) return hipErrorInvalidValue;   // flat buffers are padded to multiples of 64
    // the table must cover the slice: a cursor that ran past it would hand the tail the last range's scalars silently
    if (f.tab && ((f.first & 3) || f.first < 0 || f.tab->n < 1 || f.tab->n > AFR_OPT_MAX_RANGES || (f.first + f.n) / 4 > (long long)f.tab->end4[f.tab->n - 1]))
        return hipErrorInvalidValue;
    const long long n4 = f.n / 4;
    const dim3 grid(grid_for(n4, 256, 4096));
    with_bool(f.sumsq != nullptr, [&](auto clip) { with_opt(f.kind, [&](auto opt) {
        if (f.tab)
            hipLaunchKernelGGL((opt_groups_kernel<clip(), opt()>), grid, dim3(256), 0, s, f.p, f.g, f.m, f.v, f.shadow, n4, (unsigned)(f.first / 4), f.h.b1,
                               f.h.b2, f.h.eps, f.h.rsqrt_bc2, f.grad_scale, f.sumsq, f.max_norm, *f.tab);
        else
            hipLaunchKernelGGL((adamw_kernel<clip(), opt()>), grid, dim3(256), 0, s, f.p, f.g, f.m, f.v, f.shadow, n4, f.lr, f.h.b1, f.h.b2, f.h.eps, f.wd,
                               f.h.step, f.h.rsqrt_bc2, f.grad_scale, f.sumsq, f.max_norm);
    }); });
    return hipGetLastError();
}

// ----------------------------------------------------------------------------------- weight EMA
// e[i] = fma(p[i] - e[i], alpha, e[i]), alpha = fl(1 - decay) from the host (afr_set_ema / afr_op_ema): the exponential moving
// average of the weights, one pass over the whole flat buffer AFTER the optimizer step (the padding of e follows the padding of p).
// 12 bytes per element: e is streamed -- loaded and stored non-temporally, nothing reads it again before the next update -- while p
// was just written by the optimizer and is what the next forward reads.  p[i] == e[i] gives e[i] back bit for bit (0 * alpha + e).
// sumsq (NULL = none): the clipping plan's sum of squared gradients; a non-finite one means the optimizer step was skipped, and the
// EMA then stays as it is too.  Every lane loads the one word, as in adamw_kernel<true>.
__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ e, const float* __restrict__ p, long long n4, float alpha,
                                                  const float* __restrict__ sumsq) {
    if (sumsq && !finite_f(*sumsq)) return;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4 ee = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(e) + i);
        const f32x4 pp = reinterpret_cast<const f32x4*>(p)[i];
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = __builtin_fmaf(pp[r] - ee[r], alpha, ee[r]);
        __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(e) + i);
    }
}
hipError_t afr_launch_ema(float* e, const float* p, long long n, float decay, const float* sumsq, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (n & 3) return hipErrorInvalidValue;   // flat buffers are padded to multiples of 64
    hipLaunchKernelGGL(ema_kernel, dim3(grid_for(n / 4, 256, 4096)), dim3(256), 0, s, e, p, n / 4, 1.0f - decay, sumsq);
    return hipGetLastError();
}

// ------------------------------------------------------------------------ global gradient norm
// *out = sum of g[i]^2 over the ELEMENTS of the parameter tensors inside [lo, hi) of the flat gradient buffer, from a device table
// of (offset, numel) segments, each clipped to the range (segments start on multiples of 64 elements and lo, hi are multiples of
// 4, so a clipped segment starts 16-byte aligned).  The 64-element padding between tensors is never read: the fused glyph step,
// the slab reduces and the gradient accumulation leave arbitrary values there.
// A block belongs to ONE segment (as in the grouped reduce: a walk of every segment by every block paid one memory latency per
// tensor, 21 us for C3's 8.5 MB): segment k gets ceil(n4_k / (256 q)) blocks, at least one, of q float4 per lane; the launcher
// picks the smallest power of two q that fits the grid cap and the blocks find their segment by the same count.  16-byte loads,
// four in flight per lane; scalar loads for the <= 3 elements of a tail (the pixel head's bias has ONE element).
// Fixed order: four FMA accumulators per lane (one per float4 component), (a0 + a1) + (a2 + a3), wave shuffle, the four waves
// through LDS, one partial per block; the last block to arrive adds the partials in block order -- loss_block_finish's hand-off
// (write-through partial store, drained, agent-scope ticket; the reader loads with agent-scope atomics; cdna_hip_programming.md
// Guideline 16 R1) -- and writes the sum, the statistics and, for a non-finite sum, the error bit.  No float atomics.
constexpr int SUMSQ_MAX_SEGS = 256;
static inline long long sumsq_seg_blocks(long long numel, int qshift) {          // host twin of the kernel's count
    if (numel <= 0) return 0;
    const long long nb = ((numel >> 2) + (256ll << qshift) - 1) >> (8 + qshift);
    return nb ? nb : 1;
}
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, const SumsqSeg* __restrict__ segs, int nseg,
                                                         long long lo, long long hi, int qshift, float* __restrict__ partial,
                                                         unsigned* __restrict__ counter, float* __restrict__ out,
                                                         float* __restrict__ stats, float gscale_abs, float max_norm, uint32_t* err) {
    __shared__ long long sb[SUMSQ_MAX_SEGS], sn[SUMSQ_MAX_SEGS];      // the clipped segments: first element, elements
    __shared__ float sh[256];
    __shared__ unsigned ticket;
    if ((int)threadIdx.x < nseg) {
        const SumsqSeg sg = segs[threadIdx.x];
        const long long b = max(sg.off, lo), e = min(sg.off + sg.numel, hi);
        sb[threadIdx.x] = b; sn[threadIdx.x] = e > b ? e - b : 0;
    }
    __syncthreads();
    const long long per = 256ll << qshift;                            // float4 per block
    long long j = blockIdx.x, n = 0;
    const float* src = g;
    for (int k = 0; k < nseg; ++k) {
        const long long nk = sn[k];
        if (nk == 0) continue;
        long long nb = ((nk >> 2) + per - 1) >> (8 + qshift);
        if (nb == 0) nb = 1;
        if (j < nb) { src = g + sb[k]; n = nk; break; }
        j -= nb;
    }
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (n > 0) {                                                      // (a block past the last segment has n = 0: it adds nothing)
        const long long n4 = n >> 2, i0 = j * per + threadIdx.x, iend = min(n4, (j + 1) * per);
        long long i = i0;
        if ((j + 1) * per <= n4 && qshift >= 2) {                     // a whole block: unconditional loads, four in flight
            for (; i < iend; i += 4 * 256) {
                float4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = reinterpret_cast<const float4*>(src)[i + u * 256];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    a0 = __builtin_fmaf(v[u].x, v[u].x, a0); a1 = __builtin_fmaf(v[u].y, v[u].y, a1);
                    a2 = __builtin_fmaf(v[u].z, v[u].z, a2); a3 = __builtin_fmaf(v[u].w, v[u].w, a3);
                }
            }
        }
        for (; i < iend; i += 256) {
            const float4 v = reinterpret_cast<const float4*>(src)[i];
            a0 = __builtin_fmaf(v.x, v.x, a0); a1 = __builtin_fmaf(v.y, v.y, a1);
            a2 = __builtin_fmaf(v.z, v.z, a2); a3 = __builtin_fmaf(v.w, v.w, a3);
        }
        const long long t = (n4 << 2) + threadIdx.x;                 // tail: lanes 0..2 of the segment's first block
        if (j == 0 && t < n) { const float x = src[t]; a0 = __builtin_fmaf(x, x, a0); }
    }
    const float lsum = wave_sum((a0 + a1) + (a2 + a3));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = lsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_store(partial + blockIdx.x, (sh[0] + sh[1]) + (sh[2] + sh[3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (ticket != gridDim.x - 1) return;
    float a = 0.f;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += 256)
        a += __hip_atomic_load(partial + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float ss = sh[0];
        out[0] = ss;
        float tn;
        const float coef = clip_coef(ss, gscale_abs, max_norm, tn);
        if (stats) { stats[0] = tn; stats[1] = coef; }
        if (err && !finite_f(ss)) atomicOr(err, AFR_ERR_GRAD_NONFINITE);
        __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-arm for the next call
    }
}
hipError_t afr_launch_grad_sumsq(const float* g, const SumsqSeg* segs, const SumsqSeg* segs_host, int nseg, long long lo, long long hi,
                                 float* scratch, float* out, float* stats, float grad_scale, float max_norm, uint32_t* err, hipStream_t s) {
    if (lo < 0 || hi < lo || ((lo | hi) & 3) || nseg < 0 || nseg > SUMSQ_MAX_SEGS) return hipErrorInvalidValue;
    int qshift = 0;
    long long blocks = 0;
    for (;; ++qshift) {              // the smallest power of two of float4 per lane whose block count fits the cap
        blocks = 0;
        for (int k = 0; k < nseg; ++k) {
            const long long b = std::max(segs_host[k].off, lo), e = std::min(segs_host[k].off + segs_host[k].numel, hi);
            blocks += sumsq_seg_blocks(e - b, qshift);
        }
        if (blocks <= AFR_SUMSQ_MAX_BLOCKS) break;
    }
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks ? (unsigned)blocks : 1u), dim3(256), 0, s, g, segs, nseg, lo, hi, qshift, scratch,
                       reinterpret_cast<unsigned*>(scratch + AFR_SUMSQ_COUNTER), out, stats, fabsf(grad_scale), max_norm, err);
    return hipGetLastError();
}

// ----------------------------------------------------------------------- per-tensor statistics
// One afr_tensor_stat (include/afr.h) per segment of the same (offset, numel) table: sum of x^2 and of x over the FINITE elements,
// their minimum and maximum, and the counts of NaN, infinite and zero elements; x = a[i], or a[i] - minus[i] in f32.  Only the
// segments' elements are read, never the padding between them.  Two launches, no atomics, no communication between blocks:
//   tstats_partial_kernel  a block owns ONE chunk of AFR_TSTATS_CHUNK elements of ONE segment (a segment of n elements has
//       max(1, ceil(n / CHUNK)) chunks; the block finds its pair by grad_sumsq_kernel's count).  Lane l takes the float4 l, l + 256,
//       ... of the chunk in ascending order, 16-byte loads, four in flight (eight with minus); component c of every float4 goes to
//       the lane's accumulator pair c: q_c = fmaf(x, x, q_c), s_c = s_c + x.  The <= 3 elements behind the segment's last whole
//       float4 are loaded as scalars by lanes 0..2 of the segment's LAST chunk, into pair 0, after that lane's float4s.  Then
//       (q0 + q1) + (q2 + q3), likewise s; the wave butterfly (offsets 32, 16, 8, 4, 2, 1); the four waves through LDS as
//       (w0 + w1) + (w2 + w3); one 32-byte record per block, a plain vector store.
//   tstats_finish_kernel   one wave per segment: lane l adds the partials of chunks l, l + 64, ... in ascending order, then the
//       same butterfly, and lane 0 writes the record.
// A record therefore depends on its segment's elements only -- not on the offset, the other segments or the grid -- and repeats
// bit for bit.  Classification is by bit pattern (exponent all ones: infinity or NaN; no bit below the sign: zero), so the counts
// do not depend on the denormal mode; minimum and maximum are taken on an order-preserving integer key of the bits for the same
// reason (and come out as -0 < +0).  A non-finite element adds 0 to both sums and leaves minimum and maximum alone.
static_assert(AFR_TSTATS_MAX_SEGS == SUMSQ_MAX_SEGS, "one table serves the norm and the statistics");
static_assert(sizeof(afr_tensor_stat) == 32 && AFR_TSTATS_CHUNK % (4 * 4 * 256) == 0, "two 16-byte stores per record; whole trips of four loads");
constexpr int TSTATS_C4 = AFR_TSTATS_CHUNK / 4;                          // float4 per chunk
// the segment table as the kernels take it: the plan's device array, or by value (offsets in float4, both 32-bit: 2 KiB of argument)
struct TStatTabDev { const SumsqSeg* segs; };
struct TStatTabVal { unsigned off4[AFR_TSTATS_MAX_SEGS], numel[AFR_TSTATS_MAX_SEGS]; };
__device__ __forceinline__ void tstat_seg(const TStatTabDev& t, int k, long long& off, unsigned& n) { const SumsqSeg sg = t.segs[k]; off = sg.off; n = (unsigned)sg.numel; }
__device__ __forceinline__ void tstat_seg(const TStatTabVal& t, int k, long long& off, unsigned& n) { off = 4ll * t.off4[k]; n = t.numel[k]; }
__device__ __forceinline__ unsigned tstat_chunks(unsigned n) { return n ? (unsigned)(((unsigned long long)n + AFR_TSTATS_CHUNK - 1) / AFR_TSTATS_CHUNK) : 1u; }
// unsigned key with the order of the floats (-inf < -FLT_MAX < -0 < +0 < FLT_MAX < +inf; NaNs beyond either infinity), and back
__device__ __forceinline__ unsigned tstat_key(unsigned bits) { return bits ^ ((unsigned)((int)bits >> 31) | 0x80000000u); }
__device__ __forceinline__ unsigned tstat_unkey(unsigned k) { return (k & 0x80000000u) ? k ^ 0x80000000u : ~k; }
constexpr unsigned TSTAT_KEY_LOWEST = 0x00800000u, TSTAT_KEY_HIGHEST = 0xff7fffffu;      // the keys of -FLT_MAX and FLT_MAX
struct TStatAcc {
    float q[4] = {0.f, 0.f, 0.f, 0.f}, s[4] = {0.f, 0.f, 0.f, 0.f};
    unsigned kmin = 0xffffffffu, kmax = 0u, n_nan = 0u, n_inf = 0u, n_zero = 0u;
    __device__ __forceinline__ void add(float x, int c) {
        const unsigned bits = __float_as_uint(x), mag = bits & 0x7fffffffu;
        const bool fin = mag < 0x7f800000u;
        const float xf = fin ? x : 0.f;
        q[c] = __builtin_fmaf(xf, xf, q[c]);
        s[c] += xf;
        const unsigned k = tstat_key(bits);
        kmin = min(kmin, fin ? k : 0xffffffffu);
        kmax = max(kmax, fin ? k : 0u);
        n_nan += mag > 0x7f800000u; n_inf += mag == 0x7f800000u; n_zero += mag == 0u;
    }
    __device__ __forceinline__ void add4(const float4& v) { add(v.x, 0); add(v.y, 1); add(v.z, 2); add(v.w, 3); }
};
__device__ __forceinline__ unsigned wave_sum_u(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned wave_min_u(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned wave_max_u(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}
// the record of (sums, keys, counts): minimum +inf / maximum -inf when no finite element was met
__device__ __forceinline__ void tstat_store(afr_tensor_stat* dst, float q, float s, unsigned kmin, unsigned kmax, unsigned n_nan, unsigned n_inf,
                                            unsigned n_zero, unsigned numel) {
    const unsigned mn = kmin > TSTAT_KEY_HIGHEST ? 0x7f800000u : tstat_unkey(kmin), mx = kmax < TSTAT_KEY_LOWEST ? 0xff800000u : tstat_unkey(kmax);
    uint4* d = reinterpret_cast<uint4*>(dst);
    d[0] = make_uint4(__float_as_uint(q), __float_as_uint(s), mn, mx);
    d[1] = make_uint4(n_nan, n_inf, n_zero, numel);
}
template <bool MINUS, class Tab>
__global__ __launch_bounds__(256) void tstats_partial_kernel(const float* __restrict__ a, const float* __restrict__ minus, Tab tab, int nseg,
                                                             afr_tensor_stat* __restrict__ partial) {
    __shared__ long long sb[AFR_TSTATS_MAX_SEGS];                     // the segments: first element, elements
    __shared__ unsigned sn[AFR_TSTATS_MAX_SEGS];
    __shared__ float shf[2][4];
    __shared__ unsigned shu[5][4];
    if ((int)threadIdx.x < nseg) {
        long long off;
        unsigned numel;
        tstat_seg(tab, threadIdx.x, off, numel);
        sb[threadIdx.x] = off; sn[threadIdx.x] = numel;
    }
    __syncthreads();
    long long j = blockIdx.x, base = 0;                               // (the grid is the sum of the counts: every block finds its pair)
    unsigned n = 0;
    for (int k = 0; k < nseg; ++k) {
        const unsigned nb = tstat_chunks(sn[k]);
        if (j < nb) { base = sb[k]; n = sn[k]; break; }
        j -= nb;
    }
    const long long n4 = n >> 2, c0 = j * TSTATS_C4, c1 = min(n4, c0 + TSTATS_C4);      // this chunk's float4s: [c0, c1)
    const float4* src = reinterpret_cast<const float4*>(a + base);
    const float4* sub = MINUS ? reinterpret_cast<const float4*>(minus + base) : nullptr;
    auto diff = [](float4 v, const float4& w) { v.x -= w.x; v.y -= w.y; v.z -= w.z; v.w -= w.w; return v; };
    TStatAcc acc;
    long long i = c0 + threadIdx.x;
    if (c1 - c0 == TSTATS_C4) {                                       // a whole chunk: unconditional loads
        for (int t = 0; t < TSTATS_C4 / 256; t += 4, i += 4 * 256) {
            float4 v[4], w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = src[i + u * 256];
            if constexpr (MINUS) {
#pragma unroll
                for (int u = 0; u < 4; ++u) w[u] = sub[i + u * 256];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc.add4(MINUS ? diff(v[u], w[u]) : v[u]);
        }
    } else {
        for (; i < c1; i += 256) acc.add4(MINUS ? diff(src[i], sub[i]) : src[i]);
    }
    const long long last0 = (long long)(tstat_chunks(n) - 1) * AFR_TSTATS_CHUNK;      // first element of the segment's last chunk
    const long long t = (n4 << 2) + threadIdx.x;                      // tail: lanes 0..2 of that chunk's block
    if (j * (long long)AFR_TSTATS_CHUNK == last0 && t < n) acc.add(MINUS ? a[base + t] - minus[base + t] : a[base + t], 0);
    const long long e0 = j * (long long)AFR_TSTATS_CHUNK;
    const unsigned mine = n > e0 ? (unsigned)min((long long)AFR_TSTATS_CHUNK, (long long)n - e0) : 0u;      // elements of this chunk

    const float q = wave_sum((acc.q[0] + acc.q[1]) + (acc.q[2] + acc.q[3])), s = wave_sum((acc.s[0] + acc.s[1]) + (acc.s[2] + acc.s[3]));
    const unsigned kmin = wave_min_u(acc.kmin), kmax = wave_max_u(acc.kmax);
    const unsigned n_nan = wave_sum_u(acc.n_nan), n_inf = wave_sum_u(acc.n_inf), n_zero = wave_sum_u(acc.n_zero);
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        shf[0][w] = q; shf[1][w] = s;
        shu[0][w] = kmin; shu[1][w] = kmax; shu[2][w] = n_nan; shu[3][w] = n_inf; shu[4][w] = n_zero;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        tstat_store(partial + blockIdx.x, (shf[0][0] + shf[0][1]) + (shf[0][2] + shf[0][3]), (shf[1][0] + shf[1][1]) + (shf[1][2] + shf[1][3]),
                    min(min(shu[0][0], shu[0][1]), min(shu[0][2], shu[0][3])), max(max(shu[1][0], shu[1][1]), max(shu[1][2], shu[1][3])),
                    (shu[2][0] + shu[2][1]) + (shu[2][2] + shu[2][3]), (shu[3][0] + shu[3][1]) + (shu[3][2] + shu[3][3]),
                    (shu[4][0] + shu[4][1]) + (shu[4][2] + shu[4][3]), mine);
}
template <class Tab>
__global__ __launch_bounds__(256) void tstats_finish_kernel(Tab tab, int nseg, const afr_tensor_stat* __restrict__ partial,
                                                            afr_tensor_stat* __restrict__ out) {
    const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);      // one wave per segment
    if (t >= nseg) return;
    long long off;
    unsigned n, first = 0;                                            // first: the chunks of the segments in front of t
    for (int k = lane; k < t; k += 64) { tstat_seg(tab, k, off, n); first += tstat_chunks(n); }
    first = wave_sum_u(first);
    tstat_seg(tab, t, off, n);
    const unsigned chunks = tstat_chunks(n);
    float q = 0.f, s = 0.f;
    unsigned kmin = 0xffffffffu, kmax = 0u, n_nan = 0u, n_inf = 0u, n_zero = 0u, numel = 0u;
    for (unsigned c = lane; c < chunks; c += 64) {
        const uint4* r = reinterpret_cast<const uint4*>(partial + first + c);
        const uint4 lo = r[0], hi = r[1];
        q += __uint_as_float(lo.x); s += __uint_as_float(lo.y);
        kmin = min(kmin, tstat_key(lo.z)); kmax = max(kmax, tstat_key(lo.w));
        n_nan += hi.x; n_inf += hi.y; n_zero += hi.z; numel += hi.w;
    }
    q = wave_sum(q); s = wave_sum(s);
    kmin = wave_min_u(kmin); kmax = wave_max_u(kmax);
    n_nan = wave_sum_u(n_nan); n_inf = wave_sum_u(n_inf); n_zero = wave_sum_u(n_zero); numel = wave_sum_u(numel);
    if (lane == 0) tstat_store(out + t, q, s, kmin, kmax, n_nan, n_inf, n_zero, numel);
}
hipError_t afr_launch_tensor_stats(const float* a, const float* minus, const SumsqSeg* segs_dev, const SumsqSeg* segs_host, int nseg,
                                   afr_tensor_stat* out, afr_tensor_stat* partial, hipStream_t s) {
    if (nseg < 1 || nseg > AFR_TSTATS_MAX_SEGS) return hipErrorInvalidValue;
    long long blocks = 0;
    TStatTabVal val;
    for (int k = 0; k < nseg; ++k) {
        const SumsqSeg& sg = segs_host[k];
        if (sg.off < 0 || (sg.off & 3) || (sg.off >> 2) > 0xffffffffll || sg.numel < 0 || sg.numel > 0xffffffffll) return hipErrorInvalidValue;
        val.off4[k] = (unsigned)(sg.off >> 2); val.numel[k] = (unsigned)sg.numel;
        blocks += afr_tstats_seg_blocks(sg.numel);
    }
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    auto go = [&](const auto& tab) {
        using Tab = std::decay_t<decltype(tab)>;
        with_bool(minus != nullptr, [&](auto m) {
            hipLaunchKernelGGL((tstats_partial_kernel<m(), Tab>), dim3((unsigned)blocks), dim3(256), 0, s, a, minus, tab, nseg, partial);
        });
        if (hipError_t e = hipGetLastError()) return e;           // (no finish over partials that were never written)
        hipLaunchKernelGGL((tstats_finish_kernel<Tab>), dim3((unsigned)((nseg + 3) / 4)), dim3(256), 0, s, tab, nseg, partial, out);
        return hipGetLastError();
    };
    return segs_dev ? go(TStatTabDev{segs_dev}) : go(val);
}

// ------------------------------------------------------------------------------- f32 -> bf16
__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst,
                                                          long long n) {
    const long long n4 = n >> 2;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 a = reinterpret_cast<const float4*>(src)[i];
        bf16x4 o = {(bf16_t)a.x, (bf16_t)a.y, (bf16_t)a.z, (bf16_t)a.w};
        reinterpret_cast<bf16x4*>(dst)[i] = o;
    }
    for (long long i = (n4 << 2) + blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        dst[i] = (bf16_t)src[i];
}
hipError_t afr_launch_f32_to_bf16(const float* src, bf16_t* dst, long long n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, s, src, dst, n);
    return hipGetLastError();
}

// -------------------------------------------------------------------------------- f32 -> fp8
// dst = e4m3(src / scale), OCP e4m3fn (gfx950's native fp8: bias 7, max 448, no infinities), round to nearest even, saturating
// at +-448 (the infinities included); a NaN stays a NaN (byte & 0x7F == 0x7F).  The quotient is the correctly rounded float32
// division (include/afr.h: the byte is that of torch's cast of src / scale; x * (1.f / scale) is another float32 and rounds to
// another byte next to a tie).  The per-tensor scale is the caller's (max |src| / 448 is the usual choice).
// (the clamp is two ordered comparisons, not fminf / fmaxf: those return their other operand for a NaN, which would leave as -448)
__device__ __forceinline__ float fp8_operand(float x, float scale) {
    const float q = x / scale;
    return q > 448.f ? 448.f : q < -448.f ? -448.f : q;
}
__global__ __launch_bounds__(256) void f32_to_fp8_kernel(const float* __restrict__ src, unsigned char* __restrict__ dst, long long n,
                                                         float scale) {
    const long long n4 = n >> 2;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 a = reinterpret_cast<const float4*>(src)[i];
        int w = 0;
        w = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_operand(a.x, scale), fp8_operand(a.y, scale), w, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_operand(a.z, scale), fp8_operand(a.w, scale), w, true);
        reinterpret_cast<int*>(dst)[i] = w;
    }
    for (long long i = (n4 << 2) + blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float x = fp8_operand(src[i], scale);
        dst[i] = (unsigned char)(__builtin_amdgcn_cvt_pk_fp8_f32(x, x, 0, false) & 0xFF);
    }
}
hipError_t afr_launch_f32_to_fp8(const float* src, unsigned char* dst, long long n, float scale, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(f32_to_fp8_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, s, src, dst, n, scale);
    return hipGetLastError();
}

// -------------------------------------------------------------------- clamp output (eval path)
// y = clamp(u, 0, 1) as float32: the model's output activation (reference model.py:156,202); LOSS_BCE: y = sigmoid(u)
template <typename T, int LOSS = LOSS_MSE>
__global__ __launch_bounds__(256) void clamp_out_kernel(const T* __restrict__ u, float* __restrict__ y, long long n) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        if constexpr (LOSS == LOSS_BCE) y[i] = sigmoid_f((float)u[i]);
        else y[i] = fminf(fmaxf((float)u[i], 0.f), 1.f);
    }
}
hipError_t afr_launch_clamp_out(int act_dtype, const void* u, float* y, long long n, hipStream_t s, int loss_kind) {
    if (n <= 0) return hipSuccess;
    with_act(act_dtype == AFR_BF16, [&](auto t) { with_loss(loss_kind, [&](auto loss) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((clamp_out_kernel<T, loss()>), dim3(grid_for(n, 256)), dim3(256), 0, s, (const T*)u, y, n);
    }); });
    return hipGetLastError();
}

// du = dy * [0 <= u <= 1], in place over u: torch.clamp's backward (reference model.py:156) for a caller-side loss
// LOSS_BCE (sigmoid head): du = dy * y * (1 - y) with y = sigmoid(u) recomputed from the stored u
template <typename T, int LOSS = LOSS_MSE>
__global__ __launch_bounds__(256) void clamp_bwd_kernel(T* __restrict__ u, const float* __restrict__ dy, long long n) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float uv = (float)u[i];
        if constexpr (LOSS == LOSS_BCE) {
            const float y = sigmoid_f(uv);
            u[i] = (T)(dy[i] * y * (1.f - y));
        } else u[i] = (T)((uv >= 0.f && uv <= 1.f) ? dy[i] : 0.f);
    }
}
hipError_t afr_launch_clamp_bwd(int act_dtype, void* u, const float* dy, long long n, hipStream_t s, int loss_kind) {
    if (n <= 0) return hipSuccess;
    with_act(act_dtype == AFR_BF16, [&](auto t) { with_loss(loss_kind, [&](auto loss) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((clamp_bwd_kernel<T, loss()>), dim3(grid_for(n, 256)), dim3(256), 0, s, (T*)u, dy, n);
    }); });
    return hipGetLastError();
}

// ------------------------------------------------------------------------- MSE loss + gradient
// loss = sum((clamp(u,0,1) - t)^2) / mean_elems ;  du = 2 (y - t) / mean_elems * [0 <= u <= 1]
// (reference model.py:156,268-270 and the first step of loss.backward(), model.py:309).
// 8 pixels per lane per iteration: u as 2 x 16 B (f32) or 16 B (bf16), target as 8 B (u8) or 2 x 16 B (f32).
// du may alias u.  Per-lane sums -> wave shuffle -> LDS -> one partial per block -> fixed-order finisher.
// ROWS: the targets of row r of u are row rowmap[r] of tgt (a resident data set read in place; cols8 = groups of 8 pixels per
// row): the same walk over u, the target group addressed as (row, column group) with 64-bit arithmetic.
// LOSS_BCE: the same walk, loads, stores and block finish with loss = sum(max(u,0) - t u + log1p(exp(-|u|))) / mean_elems and
// du = (sigmoid(u) - t) / mean_elems (bce_logits_elem): F.binary_cross_entropy_with_logits on the sigmoid head's logits.
template <typename T, typename TT, bool ROWS, int LOSS = LOSS_MSE>
__global__ __launch_bounds__(256) void mse_grad_kernel(const T* __restrict__ u, const TT* __restrict__ tgt,
                                                       T* __restrict__ du, long long n8, float inv_n,
                                                       float* __restrict__ partial, unsigned* __restrict__ counter,
                                                       float* __restrict__ loss_accum, const int* __restrict__ rowmap, int cols8) {
    float lsum = 0.f;
    const float g2 = 2.f * inv_n;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        size_t ti = (size_t)i;                   // the target's group of 8 pixels
        if (ROWS) {
            const long long r = i / cols8;
            ti = (size_t)rowmap[r] * (size_t)cols8 + (size_t)(i - r * cols8);
        }
        float uu[8], tt[8];
        if (sizeof(T) == 4) {
            const float4 a = reinterpret_cast<const float4*>(u)[2 * i], b = reinterpret_cast<const float4*>(u)[2 * i + 1];
            uu[0] = a.x; uu[1] = a.y; uu[2] = a.z; uu[3] = a.w; uu[4] = b.x; uu[5] = b.y; uu[6] = b.z; uu[7] = b.w;
        } else {
            const bf16x8 a = reinterpret_cast<const bf16x8*>(u)[i];
#pragma unroll
            for (int k = 0; k < 8; ++k) uu[k] = (float)a[k];
        }
        if (sizeof(TT) == 1) {
            targets_u8x8<false>(reinterpret_cast<const uint2*>(tgt)[ti], nullptr, tt);
        } else {
            const float4 a = reinterpret_cast<const float4*>(tgt)[2 * ti], b = reinterpret_cast<const float4*>(tgt)[2 * ti + 1];
            tt[0] = a.x; tt[1] = a.y; tt[2] = a.z; tt[3] = a.w; tt[4] = b.x; tt[5] = b.y; tt[6] = b.z; tt[7] = b.w;
        }
        float dd[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) lsum += loss_elem<LOSS>(uu[k], tt[k], inv_n, g2, dd[k]);
        if (sizeof(T) == 4) {
            reinterpret_cast<float4*>(du)[2 * i] = make_float4(dd[0], dd[1], dd[2], dd[3]);
            reinterpret_cast<float4*>(du)[2 * i + 1] = make_float4(dd[4], dd[5], dd[6], dd[7]);
        } else {
            bf16x8 o;
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = (bf16_t)dd[k];
            reinterpret_cast<bf16x8*>(du)[i] = o;
        }
    }
    __shared__ float wsum[4];
    __shared__ float sh[256];
    lsum = wave_sum(lsum);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = lsum;
    __syncthreads();
    loss_block_finish((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]), partial, counter, loss_accum, inv_n, sh);
}
int afr_mse_blocks(long long rows, long long cols) { return grid_for(rows * cols / 8, 256, 1024); }
hipError_t afr_launch_mse_grad(int act_dtype, const void* u, void* du, long long rows, long long cols, const LossArgs& l, hipStream_t s) {
    const long long n = rows * cols;
    if (n <= 0) return hipSuccess;
    if ((n & 7) || (l.rowmap && (cols & 7))) return hipErrorInvalidValue;
    const dim3 g(afr_mse_blocks(rows, cols)), b(256);
    with_act(act_dtype == AFR_BF16, [&](auto ta) { with_bool(l.tdtype == AFR_TARGET_U8, [&](auto u8) { with_bool(l.rowmap != nullptr, [&](auto tr) {
        with_loss(l.kind, [&](auto loss) {
            using T = typename decltype(ta)::type;
            using TT = std::conditional_t<u8(), uint8_t, float>;
            hipLaunchKernelGGL((mse_grad_kernel<T, TT, tr(), loss()>), g, b, 0, s, (const T*)u, (const TT*)l.target, (T*)du, n / 8, l.inv_n, l.partial,
                               l.counter, l.loss_accum, l.rowmap, tr() ? (int)(cols / 8) : 0);
        });
    }); }); });
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ evaluation rows
// One read-only pass over the saved pre-activation u [rows][cols] (afr_eval / afr_op_eval): per batch row b
//   q[b][i]      = (uint8)(y * 255.0f), truncating (helpers.binary_array_to_image), y = the plan's head of u (clamp_out_kernel's
//                  inlines: clamp(u,0,1), or sigmoid_f(u) for LOSS_BCE); a NaN u gives level 0
//   loss_rows[b] = (sum_i term(u, t)) / cols, term = what loss_elem<LOSS> returns (called with inv_n = g2 = 0, du dropped), t as the
//                  loss kernels form it (k / 255.0f, or the float target); a NaN u makes its row's loss NaN
//   stats[b][4]  = #(d >= 1), #(d >= 2), max d, #((q >= 128) != (t8 >= 128)) with d = |q - t8|, t8 = k or rintf(t * 255.f) in 0..255
// mse_grad_kernel's loads (8 pixels per lane per group: u as 2 x 16 B or 16 B, targets as 8 B or 2 x 16 B, the ROWS target row
// addressed with 64-bit arithmetic) and 8-byte stores of q.  Absent outputs: HAS_T false carries no target code, HAS_Q false no
// store; loss_rows / stats alone are tested once per row.
// A row is owned by ONE wave (BLOCK false: cols <= EVAL_WAVE_COLS, row = 4 * block + wave) or ONE 256-lane workgroup (BLOCK true);
// rows beyond the grid are taken in a loop.  Nothing passes between workgroups: no tickets, no atomics.
// SUMMATION ORDER of loss_rows[b] (f32, every addition rounded on its own, no contraction), L = 64 lanes (wave) or 256 (block):
//   1. lane l starts at 0.f and adds the terms of its groups g = l, l + L, l + 2L, ... (< cols / 8) in ascending g, the 8 pixels of a
//      group in ascending pixel order: a chain of 8 * ceil((cols/8 - l) / L) additions;
//   2. wave_sum: 6 butterfly steps, v += shfl_xor(v, o) for o = 32, 16, 8, 4, 2, 1 (lanes without a group hold 0.f);
//   3. BLOCK only: ((w0 + w1) + w2) + w3, the four waves in wave order;
//   4. one division by (float)cols.
// Longest chain of additions: D(cols) = 8 * ceil(cols / (8 L)) + 6 (+ 3 for BLOCK).  A row's results depend on the row's data alone.
constexpr int EVAL_WAVE_COLS = 2048;      // up to here a wave owns a row (<= 4 groups per lane); beyond, a workgroup does
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
template <typename T, typename TT, bool ROWS, int LOSS, bool BLOCK, bool HAS_T, bool HAS_Q>
__global__ __launch_bounds__(256) void eval_rows_kernel(const T* __restrict__ u, const TT* __restrict__ tgt, const int* __restrict__ rowmap,
                                                        long long rows, int cols8, float* __restrict__ loss_rows,
                                                        uint32_t* __restrict__ stats, uint8_t* __restrict__ q) {
    constexpr int L = BLOCK ? 256 : 64;
    const int lane = BLOCK ? (int)threadIdx.x : (int)(threadIdx.x & 63), wave = threadIdx.x >> 6;
    __shared__ float wf[4];
    __shared__ unsigned wu[4][4];
    const float fcols = (float)(8 * cols8);
    const long long rstep = BLOCK ? (long long)gridDim.x : 4ll * gridDim.x;
    for (long long b = BLOCK ? (long long)blockIdx.x : 4ll * blockIdx.x + wave; b < rows; b += rstep) {
        const size_t ub = (size_t)b * (size_t)cols8;                   // the row's first group of 8 pixels
        size_t tb = ub;
        if constexpr (HAS_T && ROWS) tb = (size_t)rowmap[b] * (size_t)cols8;
        float lsum = 0.f;
        unsigned c1 = 0, c2 = 0, mx = 0, c3 = 0;
#pragma unroll 2
        for (int g = lane; g < cols8; g += L) {
            const size_t i = ub + g;
            float uu[8];
            if (sizeof(T) == 4) {
                const float4 a = reinterpret_cast<const float4*>(u)[2 * i], c = reinterpret_cast<const float4*>(u)[2 * i + 1];
                uu[0] = a.x; uu[1] = a.y; uu[2] = a.z; uu[3] = a.w; uu[4] = c.x; uu[5] = c.y; uu[6] = c.z; uu[7] = c.w;
            } else {
                const bf16x8 a = reinterpret_cast<const bf16x8*>(u)[i];
#pragma unroll
                for (int k = 0; k < 8; ++k) uu[k] = (float)a[k];
            }
            float tt[8];
            int t8[8];
            if constexpr (HAS_T) {
                const size_t ti = tb + g;
                if (sizeof(TT) == 1) {
                    const uint2 w = reinterpret_cast<const uint2*>(tgt)[ti];
                    targets_u8x8<false>(w, nullptr, tt);
#pragma unroll
                    for (int r = 0; r < 4; ++r) { t8[r] = (int)((w.x >> (8 * r)) & 0xFF); t8[4 + r] = (int)((w.y >> (8 * r)) & 0xFF); }
                } else {
                    const float4 a = reinterpret_cast<const float4*>(tgt)[2 * ti], c = reinterpret_cast<const float4*>(tgt)[2 * ti + 1];
                    tt[0] = a.x; tt[1] = a.y; tt[2] = a.z; tt[3] = a.w; tt[4] = c.x; tt[5] = c.y; tt[6] = c.z; tt[7] = c.w;
#pragma unroll
                    for (int k = 0; k < 8; ++k) t8[k] = (int)fminf(fmaxf(rintf(tt[k] * 255.f), 0.f), 255.f);
                }
            }
            unsigned qq[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                float v;
                if constexpr (LOSS == LOSS_BCE) v = fmaxf(sigmoid_f(uu[k]) * 255.0f, 0.f);      // (fmaxf: a NaN becomes level 0)
                else v = fminf(fmaxf(uu[k], 0.f), 1.f) * 255.0f;                               // (the clamp already drops a NaN)
                qq[k] = (unsigned)v;
                if constexpr (HAS_T) {
                    float du;
                    float term = loss_elem<LOSS>(uu[k], tt[k], 0.f, 0.f, du);
                    if constexpr (LOSS == LOSS_MSE) term = uu[k] == uu[k] ? term : uu[k];       // the clamp hides a NaN: the row's loss must not
                    lsum = add_rn(lsum, term);
                    const int df = (int)qq[k] - t8[k];
                    const unsigned d = (unsigned)(df < 0 ? -df : df);
                    c1 += d >= 1u; c2 += d >= 2u; mx = max(mx, d);
                    c3 += (qq[k] >= 128u) != (t8[k] >= 128);
                }
            }
            if constexpr (HAS_Q) {
                uint2 o;
                o.x = qq[0] | (qq[1] << 8) | (qq[2] << 16) | (qq[3] << 24);
                o.y = qq[4] | (qq[5] << 8) | (qq[6] << 16) | (qq[7] << 24);
                reinterpret_cast<uint2*>(q)[i] = o;
            }
        }
        if constexpr (HAS_T) {
            lsum = wave_sum(lsum);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                c1 += __shfl_xor(c1, o, 64); c2 += __shfl_xor(c2, o, 64); c3 += __shfl_xor(c3, o, 64);
                mx = max(mx, (unsigned)__shfl_xor(mx, o, 64));
            }
            if constexpr (BLOCK) {
                if ((threadIdx.x & 63) == 0) { wf[wave] = lsum; wu[wave][0] = c1; wu[wave][1] = c2; wu[wave][2] = mx; wu[wave][3] = c3; }
                __syncthreads();
                if (threadIdx.x == 0) {
                    lsum = add_rn(add_rn(add_rn(wf[0], wf[1]), wf[2]), wf[3]);
                    c1 = wu[0][0] + wu[1][0] + wu[2][0] + wu[3][0];
                    c2 = wu[0][1] + wu[1][1] + wu[2][1] + wu[3][1];
                    mx = max(max(wu[0][2], wu[1][2]), max(wu[2][2], wu[3][2]));
                    c3 = wu[0][3] + wu[1][3] + wu[2][3] + wu[3][3];
                }
            }
            if (lane == 0) {
                if (loss_rows) loss_rows[b] = lsum / fcols;
                if (stats) *reinterpret_cast<uint4*>(stats + 4 * b) = make_uint4(c1, c2, mx, c3);
            }
            if constexpr (BLOCK) __syncthreads();          // (wf / wu are free again before the block's next row)
        }
    }
}
int afr_eval_blocks(long long rows, long long cols) {
    return cols <= EVAL_WAVE_COLS ? grid_for(rows, 4, AFR_EVAL_MAX_BLOCKS) : grid_for(rows, 1, AFR_EVAL_MAX_BLOCKS);
}
hipError_t afr_launch_eval_rows(int act_dtype, int loss_kind, const void* u, const void* target, int tdtype, const int* rowmap, long long rows,
                                long long cols, float* loss_rows, uint32_t* stats, uint8_t* q, hipStream_t s) {
    if (rows <= 0 || cols <= 0) return hipSuccess;
    if ((cols & 7) || cols / 8 > 0x7fffffffll || (!target && (loss_rows || stats || rowmap)) || (!loss_rows && !stats && !q)) return hipErrorInvalidValue;
    if (!loss_rows && !stats) target = nullptr;           // nothing needs the target: the launch that carries no target code
    const dim3 g(afr_eval_blocks(rows, cols)), b(256);
    const int cols8 = (int)(cols / 8);
    auto launch = [&](auto ta, auto tt, auto tr, auto loss, auto blk, auto ht, auto hq) {
        using T = typename decltype(ta)::type;
        using TT = typename decltype(tt)::type;
        hipLaunchKernelGGL((eval_rows_kernel<T, TT, tr(), loss(), blk(), ht(), hq()>), g, b, 0, s, (const T*)u, (const TT*)target, rowmap, rows, cols8,
                           loss_rows, stats, q);
    };
    with_act(act_dtype == AFR_BF16, [&](auto ta) { with_loss(loss_kind, [&](auto loss) { with_bool(cols > EVAL_WAVE_COLS, [&](auto blk) {
        if (!target) { launch(ta, TypeTag<uint8_t>{}, std::false_type{}, loss, blk, std::false_type{}, std::true_type{}); return; }
        with_bool(tdtype == AFR_TARGET_U8, [&](auto u8) { with_bool(rowmap != nullptr, [&](auto tr) { with_bool(q != nullptr, [&](auto hq) {
            launch(ta, TypeTag<std::conditional_t<u8(), uint8_t, float>>{}, tr, loss, blk, std::true_type{}, hq);
        }); }); });
    }); }); });
    return hipGetLastError();
}

// ------------------------------------------------------------------------- batch rows of a resident data set
// The prepare step of the afr_*_rows entry points: batch row b is data-set row rows[b].  An index outside [0, n_rows) sets
// AFR_ERR_ROW and is clamped BEFORE anything is addressed with it (as glyph_embed_kernel does for code indices).  ridx[b] is
// the narrowed index the loss kernels' row maps read; the codes x[row][0 .. Lc) and the font id are copied into the staging
// area the id consumers (sheet_fwd / glyph_embed / pixel_ctx ... and their backward kernels) are handed (sx NULL: ridx only).
__global__ __launch_bounds__(256) void dataset_rows_kernel(const int64_t* __restrict__ rows, int B, long long n_rows,
                                                           const int64_t* __restrict__ x, const int64_t* __restrict__ font, int L, int Lc,
                                                           int* __restrict__ ridx, int64_t* __restrict__ sx, int64_t* __restrict__ sfont,
                                                           uint32_t* err_flag) {
    const int per = sx ? Lc : 1;
    const long long total = (long long)B * per;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / per), l = (int)(i - (long long)b * per);
        long long r = rows[b];
        if (r < 0 || r >= n_rows) { if (l == 0) atomicOr(err_flag, AFR_ERR_ROW); r = min(max(r, 0ll), n_rows - 1); }
        if (l == 0) {
            ridx[b] = (int)r;
            if (sx && sfont && font) sfont[b] = font[r];
        }
        if (sx) sx[(size_t)b * Lc + l] = x[(size_t)r * L + l];
    }
}
hipError_t afr_launch_dataset_rows(const int64_t* rows, int B, long long n_rows, const int64_t* x, const int64_t* font, int L, int Lc,
                                   int* ridx, int64_t* sx, int64_t* sfont, uint32_t* err_flag, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (n_rows <= 0 || n_rows > 0x7fffffffll || (sx && (Lc <= 0 || Lc > L))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dataset_rows_kernel, dim3(grid_for((long long)B * (sx ? Lc : 1), 256)), dim3(256), 0, s, rows, B, n_rows, x, font, L, Lc,
                       ridx, sx, sfont, err_flag);
    return hipGetLastError();
}

// ------------------------------------------------------------------------- glyph embedding
// out[b][:] = Emb[x[b]][:] (+ Font[font[b]][:])  -- nn.Embedding gather (reference model.py:136,167): bit-exact row
// copy in f32 mode.  An index outside [0,vocab) sets bit 0 of *err_flag (the reference raises IndexError) and is
// clamped so the kernel never reads out of bounds.
template <typename T>
__global__ __launch_bounds__(256) void glyph_embed_kernel(const float* __restrict__ emb, const float* __restrict__ femb,
                                                          const int64_t* __restrict__ x, const int64_t* __restrict__ font,
                                                          int B, int E, int vocab, int n_fonts, T* __restrict__ out,
                                                          uint32_t* err_flag) {
    const long long total = (long long)B * E;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / E), c = (int)(i % E);
        long long xi = x[b];
        if (xi < 0 || xi >= vocab) { if (c == 0) atomicOr(err_flag, 1u); xi = min(max(xi, 0ll), (long long)vocab - 1); }
        float v = emb[xi * E + c];
        if (n_fonts > 0) {
            long long fi = font ? font[b] : 0;
            if (fi < 0 || fi >= n_fonts) { if (c == 0) atomicOr(err_flag, 1u); fi = min(max(fi, 0ll), (long long)n_fonts - 1); }
            v += femb[fi * E + c];
        }
        out[i] = (T)v;
    }
}
hipError_t afr_launch_glyph_embed(int act_dtype, const float* emb, const float* font_emb, const int64_t* x,
                                  const int64_t* font, int B, int E, int vocab, int n_fonts, void* out,
                                  uint32_t* err_flag, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    dim3 g(grid_for((long long)B * E, 256)), b(256);
    if (act_dtype == AFR_BF16)
        hipLaunchKernelGGL(glyph_embed_kernel<bf16_t>, g, b, 0, s, emb, font_emb, x, font, B, E, vocab, n_fonts, (bf16_t*)out, err_flag);
    else
        hipLaunchKernelGGL(glyph_embed_kernel<float>, g, b, 0, s, emb, font_emb, x, font, B, E, vocab, n_fonts, (float*)out, err_flag);
    return hipGetLastError();
}

// First Linear folded through the embedding tables.  The glyph model feeds h0 = Emb[x] + Font[f] straight into
// fc1 (no dropout, no nonlinearity in between), and a batch of thousands of glyphs draws from only vocab + n_fonts
// distinct rows, so   fc1(h0)[b] = T[x_b] + T[vocab + f_b] + b1   with   T = [Emb; Font] . W1^T   ((vocab+n_fonts) x N1).
// The table costs (vocab+n_fonts)*N1*E MACs per step instead of B*N1*E, stays in L2, and the layer becomes a gather.
// table[r][n] = sum_k tab(r)[k] * W1[n][k].  A block stages 256 fc1 rows (coalesced, padded to E+1 in LDS) and GT_ROWS table
// rows, one thread per n; grid (ceil(rows/8), ceil(N1/256)).
constexpr int GT_ROWS = 2;    // rows per block: the kernel is latency bound, more blocks (272 at C3) beat fewer, fatter ones (8: +1.5 us)
__global__ __launch_bounds__(256) void glyph_table_kernel(const float* __restrict__ emb, const float* __restrict__ femb,
                                                          const float* __restrict__ W1, int vocab, int rows, int E, int N1,
                                                          float* __restrict__ table, bf16_t* __restrict__ w1t) {
    extern __shared__ float sm[];                         // W [256][E+1] | tab [GT_ROWS][E]
    float* Ws = sm;
    float* tab = sm + 256 * (E + 1);
    const int r0 = blockIdx.x * GT_ROWS, n0 = blockIdx.y * 256;
    const int nn = min(256, N1 - n0), nr = min(GT_ROWS, rows - r0);
    const int E4 = E >> 2;
    for (int i = threadIdx.x; i < nn * E4; i += 256) {
        const float4 v = *reinterpret_cast<const float4*>(W1 + (size_t)n0 * E + 4 * i);
        float* d = Ws + (i / E4) * (E + 1) + 4 * (i % E4);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    for (int i = threadIdx.x; i < nr * E; i += 256) {
        const int r = r0 + i / E, k = i % E;
        tab[i] = r < vocab ? emb[(size_t)r * E + k] : femb[(size_t)(r - vocab) * E + k];
    }
    __syncthreads();
    if ((int)threadIdx.x >= nn) return;
    const float* w = Ws + threadIdx.x * (E + 1);
    // the first row of blocks also leaves W1^T as bf16 [E][N1] (the fused first-layer backward reads fc1's weights k-contiguous)
    if (w1t && blockIdx.x == 0)
        for (int k = 0; k < E; ++k) w1t[(size_t)k * N1 + n0 + threadIdx.x] = (bf16_t)w[k];
    float a[GT_ROWS];
#pragma unroll
    for (int j = 0; j < GT_ROWS; ++j) a[j] = 0.f;
    for (int k = 0; k < E; ++k) {
        const float wv = w[k];
#pragma unroll
        for (int j = 0; j < GT_ROWS; ++j) a[j] = fmaf(tab[j * E + k], wv, a[j]);   // rows past nr read stale LDS; never stored
    }
    for (int j = 0; j < nr; ++j) table[(size_t)(r0 + j) * N1 + n0 + threadIdx.x] = a[j];
}
// h1[b][n] = relu(T[x_b][n] + T[vocab+f_b][n] + b1[n]), one lane per 8 consecutive n of one glyph; index checks as in
// glyph_embed_kernel.  Also leaves the backward's GEMM operand h0' [B][K0]: h0 = Emb[x_b] + Font[f_b] followed by the
// one-hot code of the two table rows the glyph used (see glyph_l1_bwd_kernel).
template <typename T>
__device__ __forceinline__ void store8(T* q, const float (&v)[8]) {
    if constexpr (sizeof(T) == 2) {
        bf16x8 w;
#pragma unroll
        for (int r = 0; r < 8; ++r) w[r] = (bf16_t)v[r];
        __builtin_nontemporal_store(w, reinterpret_cast<bf16x8*>(q));
    } else {
        const f32x4 lo = {v[0], v[1], v[2], v[3]}, hi = {v[4], v[5], v[6], v[7]};
        __builtin_nontemporal_store(lo, reinterpret_cast<f32x4*>(q));
        __builtin_nontemporal_store(hi, reinterpret_cast<f32x4*>(q) + 1);
    }
}
template <typename T>
__global__ __launch_bounds__(256) void glyph_l1_fwd_kernel(const float* __restrict__ table, const float* __restrict__ b1,
                                                           const float* __restrict__ emb, const float* __restrict__ femb,
                                                           const int64_t* __restrict__ x, const int64_t* __restrict__ font,
                                                           int B, int E, int N1, int vocab, int n_fonts, int K0,
                                                           T* __restrict__ h0, T* __restrict__ h1, uint32_t* err_flag) {
    // one glyph per threadIdx.y, its 8-column chunks of h1 (N1/8) and then of h0' (K0/8) strided over threadIdx.x: no index
    // division (a flat index over B x (N1 + K0)/8 items cost a 64-bit divide + modulo by a runtime divisor per item)
    const int c1 = N1 >> 3, c0 = K0 >> 3;
    const int b = blockIdx.x * blockDim.y + threadIdx.y;
    if (b >= B) return;
    long long xi = x[b];
    if (xi < 0 || xi >= vocab) { if (threadIdx.x == 0) atomicOr(err_flag, 1u); xi = min(max(xi, 0ll), (long long)vocab - 1); }
    long long fi = 0;
    if (n_fonts > 0) {
        fi = font ? font[b] : 0;
        if (fi < 0 || fi >= n_fonts) { if (threadIdx.x == 0) atomicOr(err_flag, 1u); fi = min(max(fi, 0ll), (long long)n_fonts - 1); }
    }
    const float* trow_c = table + (size_t)xi * N1;
    const float* trow_f = table + (size_t)(vocab + fi) * N1;
    for (int c = threadIdx.x; c < c1; c += blockDim.x) {
        float v[8];
        const int n = 8 * c;
        const float4 a0 = *reinterpret_cast<const float4*>(trow_c + n), a1 = *reinterpret_cast<const float4*>(trow_c + n + 4);
        const float4 g0 = *reinterpret_cast<const float4*>(b1 + n), g1 = *reinterpret_cast<const float4*>(b1 + n + 4);
        v[0] = a0.x + g0.x; v[1] = a0.y + g0.y; v[2] = a0.z + g0.z; v[3] = a0.w + g0.w;
        v[4] = a1.x + g1.x; v[5] = a1.y + g1.y; v[6] = a1.z + g1.z; v[7] = a1.w + g1.w;
        if (n_fonts > 0) {
            const float4 f0 = *reinterpret_cast<const float4*>(trow_f + n), f1 = *reinterpret_cast<const float4*>(trow_f + n + 4);
            v[0] += f0.x; v[1] += f0.y; v[2] += f0.z; v[3] += f0.w; v[4] += f1.x; v[5] += f1.y; v[6] += f1.z; v[7] += f1.w;
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = fmaxf(v[r], 0.f);
        store8(h1 + (size_t)b * N1 + n, v);
    }
    for (int c = threadIdx.x; c < c0; c += blockDim.x) {
        // h0' = [h0 | one-hot of x_b | one-hot of vocab + f_b | zero pad]
        float v[8];
        const int k0 = 8 * c;
        if (k0 < E) {                                     // E % 8 == 0: a chunk is all h0 or all one-hot
            const float* e = emb + (size_t)xi * E + k0;
            const float4 a0 = *reinterpret_cast<const float4*>(e), a1 = *reinterpret_cast<const float4*>(e + 4);
            v[0] = a0.x; v[1] = a0.y; v[2] = a0.z; v[3] = a0.w; v[4] = a1.x; v[5] = a1.y; v[6] = a1.z; v[7] = a1.w;
            if (n_fonts > 0) {
                const float* f = femb + (size_t)fi * E + k0;
                const float4 f0 = *reinterpret_cast<const float4*>(f), f1 = *reinterpret_cast<const float4*>(f + 4);
                v[0] += f0.x; v[1] += f0.y; v[2] += f0.z; v[3] += f0.w; v[4] += f1.x; v[5] += f1.y; v[6] += f1.z; v[7] += f1.w;
            }
        } else {
            const int r0 = k0 - E, hx = (int)xi, hf = n_fonts > 0 ? vocab + (int)fi : -1;
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = (r0 + r == hx || r0 + r == hf) ? 1.f : 0.f;
        }
        store8(h0 + (size_t)b * K0 + k0, v);
    }
}
hipError_t afr_launch_glyph_l1_fwd(int act_dtype, const float* emb, const float* font_emb, const float* W1, const float* b1,
                                   const int64_t* x, const int64_t* font, int B, int E, int N1, int vocab, int n_fonts,
                                   float* table, void* h0, void* h1, uint32_t* err_flag, hipStream_t s, void* w1t) {
    if (B <= 0) return hipSuccess;
    if ((N1 & 7) || (E & 7)) return hipErrorInvalidValue;
    const int K0 = afr_glyph_k0(E, vocab, n_fonts);
    const int rows = vocab + n_fonts;
    const size_t tlds = (size_t)(256 * (E + 1) + GT_ROWS * E) * sizeof(float);      // 35 KB at E = 32, 136 KB at the E = 128 limit
    static size_t tlds_set[16];                      // largest dynamic-LDS opt-in made so far, per device
    int dev = 0;
    if (tlds > 48 * 1024 && hipGetDevice(&dev) == hipSuccess && (dev < 0 || dev >= 16 || tlds_set[dev] < tlds)) {
        hipError_t e = hipFuncSetAttribute((const void*)glyph_table_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tlds);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 16) tlds_set[dev] = tlds;
    }
    hipLaunchKernelGGL(glyph_table_kernel, dim3((rows + GT_ROWS - 1) / GT_ROWS, (N1 + 255) / 256), dim3(256), tlds, s, emb, font_emb,
                       W1, vocab, rows, E, N1, table, (bf16_t*)w1t);
    // threads: x over a glyph's 8-column chunks (a power of two up to 128), y over glyphs; 256 threads per block
    int tx = 32;
    while (tx < 128 && tx < N1 / 8) tx *= 2;
    dim3 b(tx, 256 / tx), g((B + b.y - 1) / b.y);
    if (act_dtype == AFR_BF16)
        hipLaunchKernelGGL(glyph_l1_fwd_kernel<bf16_t>, g, b, 0, s, table, b1, emb, font_emb, x, font, B, E, N1, vocab, n_fonts, K0,
                           (bf16_t*)h0, (bf16_t*)h1, err_flag);
    else
        hipLaunchKernelGGL(glyph_l1_fwd_kernel<float>, g, b, 0, s, table, b1, emb, font_emb, x, font, B, E, N1, vocab, n_fonts, K0,
                           (float*)h0, (float*)h1, err_flag);
    return hipGetLastError();
}

// ---------------------------------------------------------------- first layer as a COMBINATION table (training steps, bf16)
// A glyph is one of vocab x max(n_fonts, 1) (character, font) combinations, so the first layer's output has at most that many
// distinct rows.  A training step therefore does not materialise h1 [B][N1] (16 MB at C3, written once and read three times:
// by the next layer's forward, by its weight gradient and by its ReLU mask) but only
//     H1c[c][n] = bf16(relu(T[x][n] + b1[n] + T[vocab + f][n]))      c = x * max(n_fonts, 1) + f   (the gather kernel's arithmetic)
//     H0c[c][k] = bf16(Emb[x][k] + Font[f][k])
//     cidx[b]   = c of glyph b
// (0.5 MB + 16 KB + 32 KB, L2-resident); the GEMM kernels that consume h1 / h0 gather their operand rows through cidx while
// staging (GemmParams::a_rowmap / b_rowmap / aux_rowmap; LDS-DMA takes a per-lane source address, so a gathered row costs
// what a dense one does).  Same values bit for bit as the gather kernel's h1 / h0, same FLOPs in every product.
// One kernel, a 1-D grid: [combination groups x row chunks of fc1 | the batch's index blocks].  A computing block takes
// CB_COMBOS combinations x CB_ROWS fc1 rows: thread (row = tid & 63, wave = tid >> 6) keeps ITS W1 row in registers (E <= CB_MAXE
// floats, read once: W1 passes L2 once per combination group, never through LDS) and runs the wave's CB_PER combinations, whose
// embedding and font rows are the same for the whole wave (uniform addresses: read through the scalar cache, an FMA operand each).
// The SAME arithmetic as the table + gather kernels, in the same order: t_c = fma chain over k from 0 of Emb[x][k] W1[n][k], t_f
// likewise for the font row, v = (t_c + b1[n]) + t_f, ReLU, one rounding to bf16 -- bit for bit the dense path's h1.
// EC: the embedding width at compile time (32, C3's) or 0 = E at run time; FONTS: n_fonts > 0.  With both known the k loop is
// one straight block, so the table rows' scalar loads are issued in batches ahead of their FMAs instead of one wait per quad.
constexpr int CB_COMBOS = 16, CB_ROWS = 64, CB_PER = 4, CB_MAXE = 40;
template <int EC, bool FONTS>
__global__ __launch_bounds__(256) void glyph_combo_kernel(const float* __restrict__ W1, const float* __restrict__ b1,
                                                          const float* __restrict__ emb, const float* __restrict__ femb,
                                                          const int64_t* __restrict__ x, const int64_t* __restrict__ font,
                                                          int B, int E_, int N1, int vocab, int n_fonts, int combo_blocks,
                                                          bf16_t* __restrict__ h1c, int ld1, bf16_t* __restrict__ h0c, int* __restrict__ cidx,
                                                          bf16_t* __restrict__ w1t, uint32_t* err_flag) {
    const int E = EC ? EC : E_;
    constexpr int KQ = (EC ? EC : CB_MAXE) / 4;           // k quads in the unrolled loops
    const int nf = max(n_fonts, 1), ncombo = vocab * nf;
    const int row_chunks = (N1 + CB_ROWS - 1) / CB_ROWS;
    if ((int)blockIdx.x >= combo_blocks * row_chunks) {   // the batch's combination indices (with the index check of the gather)
        const int b = ((int)blockIdx.x - combo_blocks * row_chunks) * 256 + threadIdx.x;
        if (b >= B) return;
        long long xi = x[b], fi = (n_fonts > 0 && font) ? font[b] : 0;
        if (xi < 0 || xi >= vocab) { atomicOr(err_flag, 1u); xi = min(max(xi, 0ll), (long long)vocab - 1); }
        if (n_fonts > 0 && (fi < 0 || fi >= n_fonts)) { atomicOr(err_flag, 1u); fi = min(max(fi, 0ll), (long long)n_fonts - 1); }
        cidx[b] = (int)(xi * nf + fi);
        return;
    }
    const int cb = blockIdx.x / row_chunks, rc = blockIdx.x - cb * row_chunks;      // a combination group's row chunks are neighbours
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = rc * CB_ROWS + (threadIdx.x & 63), c0 = cb * CB_COMBOS;
    const bool row = n < N1;
    float4 w[KQ];
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk)
        w[kk] = (4 * kk < E && row) ? *reinterpret_cast<const float4*>(W1 + (size_t)n * E + 4 * kk) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float bias = row ? b1[n] : 0.f;
    if (rc == 0)                                          // H0c = bf16(Emb[x] + Font[f]): once per combination group
        for (int i = threadIdx.x; i < min(CB_COMBOS, ncombo - c0) * E; i += 256) {
            const int c = c0 + i / E, k = i % E, xi = c / nf, fi = c - xi * nf;
            const float e = emb[(size_t)xi * E + k];
            h0c[(size_t)c * E + k] = (bf16_t)(FONTS ? e + femb[(size_t)fi * E + k] : e);
        }
    // the first combination group also leaves W1^T as bf16 [E][N1] (the fused first-layer backward reads fc1's weights
    // k-contiguous): each of its blocks the rows it holds, wave w the k quads kk = w mod 4 (128-byte stores, E / 4 per thread)
    if (w1t && cb == 0 && row) {
#pragma unroll
        for (int kk = 0; kk < KQ; ++kk)
            if (4 * kk < E && (kk & 3) == wave) {
                bf16_t* d = w1t + (size_t)(4 * kk) * N1 + n;
                d[0] = (bf16_t)w[kk].x; d[N1] = (bf16_t)w[kk].y; d[2 * (size_t)N1] = (bf16_t)w[kk].z; d[3 * (size_t)N1] = (bf16_t)w[kk].w;
            }
    }
    const int cw = c0 + wave * CB_PER;                    // this wave's combinations (those past ncombo repeat the last one; never stored)
    float tc[CB_PER], tf[CB_PER];
#pragma unroll
    for (int j = 0; j < CB_PER; ++j) {
        const int c = min(cw + j, ncombo - 1), xi = c / nf, fi = c - xi * nf;
        const float* er = emb + (size_t)xi * E;
        const float* fr = FONTS ? femb + (size_t)fi * E : er;
        tc[j] = tf[j] = 0.f;
#pragma unroll
        for (int kk = 0; kk < KQ; ++kk) {
            if (4 * kk < E) {
                const float wk[4] = {w[kk].x, w[kk].y, w[kk].z, w[kk].w};
                const float4 e4 = *reinterpret_cast<const float4*>(er + 4 * kk);
                const float ev[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                for (int u = 0; u < 4; ++u) tc[j] = fmaf(ev[u], wk[u], tc[j]);
                if (FONTS) {
                    const float4 f4 = *reinterpret_cast<const float4*>(fr + 4 * kk);
                    const float fv[4] = {f4.x, f4.y, f4.z, f4.w};
#pragma unroll
                    for (int u = 0; u < 4; ++u) tf[j] = fmaf(fv[u], wk[u], tf[j]);
                }
            }
        }
    }
    if (!row) return;
#pragma unroll
    for (int j = 0; j < CB_PER; ++j) {
        if (cw + j < ncombo) {
            float v = tc[j] + bias;
            if (FONTS) v += tf[j];
            h1c[(size_t)(cw + j) * ld1 + n] = (bf16_t)fmaxf(v, 0.f);
        }
    }
}
// combination rows + combination indices (+ W1^T) in ONE launch; h1c [vocab * max(n_fonts,1)][ld1], h0c [..][E], cidx [B]
hipError_t afr_launch_glyph_combo(const float* emb, const float* font_emb, const float* W1, const float* b1, const int64_t* x,
                                  const int64_t* font, int B, int E, int N1, int vocab, int n_fonts, float* table, void* h1c,
                                  int ld1, void* h0c, int* cidx, uint32_t* err_flag, hipStream_t s, void* w1t) {
    if (B <= 0) return hipSuccess;
    if ((N1 & 7) || (E & 7) || E > 256) return hipErrorInvalidValue;
    (void)table;
    if (E > CB_MAXE) return hipErrorInvalidValue;                      // the combination path is planned for E <= 32 .. 40
    const int ncombo = vocab * (n_fonts > 0 ? n_fonts : 1);
    const int combo_blocks = (ncombo + CB_COMBOS - 1) / CB_COMBOS;
    const dim3 grid(combo_blocks * ((N1 + CB_ROWS - 1) / CB_ROWS) + (B + 255) / 256);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, W1, b1, emb, font_emb, x, font, B, E, N1, vocab, n_fonts, combo_blocks, (bf16_t*)h1c, ld1,
                           (bf16_t*)h0c, cidx, (bf16_t*)w1t, err_flag);
    };
    if (E == 32) n_fonts > 0 ? launch(glyph_combo_kernel<32, true>) : launch(glyph_combo_kernel<32, false>);
    else n_fonts > 0 ? launch(glyph_combo_kernel<0, true>) : launch(glyph_combo_kernel<0, false>);
    return hipGetLastError();
}

// columns of h0': E + (vocab + n_fonts) rounded up to 8
int afr_glyph_k0(int E, int vocab, int n_fonts) { return E + (vocab + n_fonts + 7) / 8 * 8; }

// Backward of the folded first layer.  The weight-gradient GEMM ran against h0' = [h0 | one-hot], so its split-K slabs
// hold, per fc1 row n, both dW1[n][0..E) and S[n][r] = sum over the glyphs that used table row r of d1[b][n] -- the
// segment sums that nn.Embedding's backward (model.py:309) needs, obtained on MFMA instead of a scatter-add.  Then
//     dTab[r][k] = sum_n S[n][r] W1[n][k]        (dEmb = rows < vocab, dFont = the rest)
// replaces the B x E x N1 input-gradient GEMM and the per-glyph scatter.  A block owns GL1_ROWS fc1 rows: it sums their
// slabs (fixed order), emits the compact dW1 rows and its partial dTab, which the grouped reduce sums in block order.
constexpr int GL1_ROWS = 8, GL1_NT = 1024;
__global__ __launch_bounds__(GL1_NT) void glyph_l1_bwd_kernel(const float* __restrict__ slabs, int nslabs, long long slab_stride,
                                                              const float* __restrict__ W1, int N1, int E, int R, int K0,
                                                              float* __restrict__ dw1, float* __restrict__ dtab_part) {
    extern __shared__ float sm[];                 // S [GL1_ROWS][K0] | W [GL1_ROWS][E] | part [G-1][GL1_ROWS*K0]
    float* S = sm;
    float* W = sm + GL1_ROWS * K0;
    float* part = W + GL1_ROWS * E;
    const int n0 = blockIdx.x * GL1_ROWS;
    const int nr = min(GL1_ROWS, N1 - n0);
    const int cnt4 = nr * K0 / 4;                 // K0 % 8 == 0; <= GL1_ROWS*K0/4 float4 columns
    // the block's threads form G groups of cnt4 lanes; group g sums slabs g, g+G, ... (all loads of a lane independent),
    // then the groups are added in group order
    const int full4 = GL1_ROWS * K0 / 4;
    const int G = max(1, min(GL1_NT / full4, 8));
    const int g = threadIdx.x / full4, i = threadIdx.x % full4;
    if (g < G && i < cnt4) {
        const float* src = slabs + (size_t)n0 * K0 + 4 * i;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
        for (int z = g; z < nslabs; z += G) {
            const float4 v = *reinterpret_cast<const float4*>(src + (long long)z * slab_stride);
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
        float* dst = g == 0 ? S : part + (size_t)(g - 1) * GL1_ROWS * K0;
        *reinterpret_cast<float4*>(dst + 4 * i) = a;
    }
    for (int j = threadIdx.x; j < nr * E; j += GL1_NT) W[j] = W1[(size_t)n0 * E + j];
    __syncthreads();
    if ((int)threadIdx.x < cnt4) {
        float4 a = *reinterpret_cast<float4*>(S + 4 * threadIdx.x);
        for (int q = 1; q < G; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(part + (size_t)(q - 1) * GL1_ROWS * K0 + 4 * threadIdx.x);
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
        *reinterpret_cast<float4*>(S + 4 * threadIdx.x) = a;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < nr * E; j += GL1_NT) dw1[(size_t)n0 * E + j] = S[(j / E) * K0 + (j % E)];
    float* out = dtab_part + (size_t)blockIdx.x * R * E;
    for (int j = threadIdx.x; j < R * E; j += GL1_NT) {
        const int r = j / E, k = j % E;
        float a = 0.f;
        for (int q = 0; q < nr; ++q) a = fmaf(S[q * K0 + E + r], W[q * E + k], a);
        out[j] = a;
    }
}
int afr_glyph_l1_bwd_blocks(int N1) { return (N1 + GL1_ROWS - 1) / GL1_ROWS; }
hipError_t afr_launch_glyph_l1_bwd(const float* slabs, int nslabs, long long slab_stride, const float* W1, int N1, int E,
                                   int vocab, int n_fonts, float* dw1, float* dtab_part, hipStream_t s) {
    const int K0 = afr_glyph_k0(E, vocab, n_fonts);
    if (GL1_ROWS * K0 / 4 > GL1_NT) return hipErrorInvalidValue;      // K0 <= 512: vocab + n_fonts + E within one block
    const int G = std::max(1, std::min(GL1_NT / (GL1_ROWS * K0 / 4), 8));
    const size_t lds = ((size_t)GL1_ROWS * (K0 + E) + (size_t)(G - 1) * GL1_ROWS * K0) * sizeof(float);
    hipLaunchKernelGGL(glyph_l1_bwd_kernel, dim3(afr_glyph_l1_bwd_blocks(N1)), dim3(GL1_NT), lds, s, slabs, nslabs, slab_stride, W1, N1,
                       E, vocab + n_fonts, K0, dw1, dtab_part);
    return hipGetLastError();
}

// embedding_dense_backward (model.py:309): dEmb[x[b]] += d[b].  Deterministic, atomic-free: a block takes EMB_BWD_ROWS (32) glyph
// rows; thread (slot = tid>>5, c = tid&31) is the ONLY writer of LDS rows v with v%8 == slot, column c, and walks the
// block's rows in order.  Block partials go to slabs[block][(vocab+n_fonts)*E]; afr_launch_reduce sums them in order.
constexpr int EMB_BWD_ROWS = 32;
template <typename T>
__global__ __launch_bounds__(256) void glyph_embed_bwd_kernel(const T* __restrict__ d, const int64_t* __restrict__ x,
                                                              const int64_t* __restrict__ font, int B, int E, int vocab,
                                                              int n_fonts, float* __restrict__ slabs) {
    extern __shared__ float sm[];                  // acc [(vocab+n_fonts)][E] | tile [EMB_BWD_ROWS][E+1] | ids [EMB_BWD_ROWS] | fids [EMB_BWD_ROWS]
    const int rows_tot = vocab + n_fonts;
    const int LDT = E + 1;
    float* acc = sm;
    float* tile = sm + (size_t)rows_tot * E;
    int* ids = reinterpret_cast<int*>(tile + (size_t)EMB_BWD_ROWS * LDT);
    int* fids = ids + EMB_BWD_ROWS;
    const int b0 = blockIdx.x * EMB_BWD_ROWS;
    const int nb = min(EMB_BWD_ROWS, B - b0);
    for (int i = threadIdx.x; i < rows_tot * E; i += 256) acc[i] = 0.f;
    for (int i = threadIdx.x; i < nb * E; i += 256) tile[(i / E) * LDT + (i % E)] = (float)d[(size_t)b0 * E + i];
    if ((int)threadIdx.x < nb) {
        long long xi = x[b0 + threadIdx.x];
        ids[threadIdx.x] = (int)min(max(xi, 0ll), (long long)vocab - 1);
        long long fi = (n_fonts > 0 && font) ? font[b0 + threadIdx.x] : 0;
        fids[threadIdx.x] = (int)min(max(fi, 0ll), (long long)max(n_fonts, 1) - 1);
    }
    __syncthreads();
    const int slot = threadIdx.x >> 5, c0 = threadIdx.x & 31;
    for (int c = c0; c < E; c += 32) {
        for (int r = 0; r < nb; ++r) {
            const int v = ids[r];
            const float val = tile[r * LDT + c];
            if ((v & 7) == slot) acc[v * E + c] += val;
            if (n_fonts > 0) {
                const int f = fids[r];
                if ((f & 7) == slot) acc[(vocab + f) * E + c] += val;
            }
        }
    }
    __syncthreads();
    float* out = slabs + (size_t)blockIdx.x * rows_tot * E;
    for (int i = threadIdx.x; i < rows_tot * E; i += 256) out[i] = acc[i];
}
int afr_embed_bwd_blocks(int B) { return (B + EMB_BWD_ROWS - 1) / EMB_BWD_ROWS; }
size_t afr_glyph_embed_bwd_lds_bytes(int E, int vocab, int n_fonts) {
    return ((size_t)(vocab + n_fonts) * E + (size_t)EMB_BWD_ROWS * (E + 1)) * sizeof(float) + 2 * EMB_BWD_ROWS * sizeof(int);
}
hipError_t afr_launch_glyph_embed_bwd(int act_dtype, const void* d, const int64_t* x, const int64_t* font, int B, int E,
                                      int vocab, int n_fonts, float* slabs, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    const size_t lds = afr_glyph_embed_bwd_lds_bytes(E, vocab, n_fonts);
    if (lds > 160 * 1024) return hipErrorInvalidValue;                  // the whole table's accumulator sits in one block's LDS
    static size_t set[2][16];                        // largest dynamic-LDS opt-in made so far, per instantiation and device
    int dev = 0;
    const int ti = act_dtype == AFR_BF16 ? 1 : 0;
    if (lds > 48 * 1024 && hipGetDevice(&dev) == hipSuccess && (dev < 0 || dev >= 16 || set[ti][dev] < lds)) {
        hipError_t e = ti ? hipFuncSetAttribute((const void*)glyph_embed_bwd_kernel<bf16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
                          : hipFuncSetAttribute((const void*)glyph_embed_bwd_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 16) set[ti][dev] = lds;
    }
    dim3 g(afr_embed_bwd_blocks(B)), b(256);
    if (act_dtype == AFR_BF16)
        hipLaunchKernelGGL(glyph_embed_bwd_kernel<bf16_t>, g, b, lds, s, (const bf16_t*)d, x, font, B, E, vocab, n_fonts, slabs);
    else
        hipLaunchKernelGGL(glyph_embed_bwd_kernel<float>, g, b, lds, s, (const float*)d, x, font, B, E, vocab, n_fonts, slabs);
    return hipGetLastError();
}
