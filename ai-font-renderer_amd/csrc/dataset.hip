// dataset.hip -- the sheet data set composed on the device (afr_op_dataset_text, afr_op_compose_sheets; include/afr.h): the seeded
// text source and the wrap / pen / blit of the reference's offline generator (generate_font.ts:164-206 and :64-142), which
// datagen.py restates on the CPU with PIL.  Integer arithmetic throughout: a sheet is bit for bit what datagen.render_sheet draws.
// afr_op_sheet_char_errors runs the same layout to attribute a prediction's error to the characters that own the pixels.
#include "afr_common.h"

// ------------------------------------------------------------------------------------------- text
// One lane per sample: synth.lcg_text in integers, the walk dataset_text_kernel and dataset_text_w_kernel share.  draw(k) is
// int(rnd() * k) as (state * k) >> 32 -- state / 2^32 * k is exact in a double.  letter(draw) is the source's own part: the code of the
// next letter.  live = false draws nothing: an empty sample.  A sample writes pos <= length <= max_len <= ldx codes and zero-fills the
// rest of its row: every element of the row, once.  (dataset_text_m_kernel, whose source can fail in the middle of a text and carries
// a context from letter to letter, keeps the same walk as a loop of its own: run through this one it measured 5 % slower.)
template <class Letter>
__device__ __forceinline__ void text_walk(long long first_seed, const int64_t* __restrict__ seed_rows, const int64_t* __restrict__ out_rows,
                                          long long j, int min_len, int max_len, int64_t* __restrict__ codes, int ldx,
                                          int32_t* __restrict__ len, bool live, Letter letter) {
    uint32_t state = (uint32_t)(uint64_t)(first_seed + (seed_rows ? seed_rows[j] : j));      // the update is mod 2^32 from the start
    const long long row = out_rows ? out_rows[j] : j;
    int64_t* dst = codes + row * (long long)ldx;
    auto draw = [&](uint32_t k) -> uint32_t {
        state = state * 1664525u + 1013904223u;
        return (uint32_t)(((uint64_t)state * k) >> 32);
    };
    const int length = live ? (int)draw((uint32_t)(max_len - min_len + 1)) + min_len : 0;
    int remaining = length, pos = 0;
    while (remaining > 0) {
        const int wl = min((int)draw(10u) + 1, remaining);
        for (int i = 0; i < wl; ++i) dst[pos++] = letter(draw);
        remaining -= wl;
        if (remaining > 0) { dst[pos++] = 32; --remaining; }
    }
    for (; pos < ldx; ++pos) dst[pos] = 0;
    if (len) len[row] = length;
}

__global__ __launch_bounds__(256) void dataset_text_kernel(long long first_seed, const int64_t* __restrict__ seed_rows,
                                                           const int64_t* __restrict__ out_rows, long long n, int min_len, int max_len,
                                                           int64_t* __restrict__ codes, int ldx, int32_t* __restrict__ len) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    text_walk(first_seed, seed_rows, out_rows, j, min_len, max_len, codes, ldx, len, true, [](auto& draw) { return 65 + (int)draw(26u); });
}

hipError_t afr_launch_dataset_text(long long first_seed, const int64_t* seed_rows, const int64_t* out_rows, long long n, int min_len, int max_len,
                                   int64_t* codes, int ldx, int32_t* len, hipStream_t s) {
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(dataset_text_kernel, dim3(blocks), dim3(256), 0, s, first_seed, seed_rows, out_rows, n, min_len, max_len, codes, ldx, len);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------- weighted text
// afr_op_dataset_text_w: dataset_text_kernel with the letter drawn from a table of weights (synth.lcg_text_weighted).  The 94 inclusive
// cumulative weights go to LDS once per workgroup, padded to 128 entries with 2^32 - 1, which no draw r < total <= 2^32 - 1 reaches: the
// seven-step search then needs no bound check.  It counts the entries <= r, which is the smallest i with cum[i] > r; an entry of
// zero width (cum[i] == cum[i - 1]) is passed over with its predecessor.  A table whose total is 0 draws nothing: zero rows, bit 0 of *err.
constexpr int TXT_FIRST = 33, TXT_CODES = 94, TXT_PAD = 128;
__device__ __forceinline__ int text_search(const uint32_t* tab, uint32_t r) {
    int at = 0;
#pragma unroll
    for (int step = TXT_PAD / 2; step > 0; step >>= 1)
        if (tab[at + step - 1] <= r) at += step;
    return at;
}

__global__ __launch_bounds__(256) void dataset_text_w_kernel(long long first_seed, const int64_t* __restrict__ seed_rows,
                                                             const int64_t* __restrict__ out_rows, long long n, int min_len, int max_len,
                                                             const uint32_t* __restrict__ cum, int64_t* __restrict__ codes, int ldx,
                                                             int32_t* __restrict__ len, uint32_t* __restrict__ err) {
    __shared__ uint32_t s_cum[TXT_PAD];
    if (threadIdx.x < TXT_PAD) s_cum[threadIdx.x] = threadIdx.x < TXT_CODES ? cum[threadIdx.x] : 0xFFFFFFFFu;
    __syncthreads();
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t total = s_cum[TXT_CODES - 1];
    text_walk(first_seed, seed_rows, out_rows, j, min_len, max_len, codes, ldx, len, total != 0u,
              [&](auto& draw) { return TXT_FIRST + text_search(s_cum, draw(total)); });
    if (total == 0u && threadIdx.x == 0 && err) atomicOr(err, AFR_ERR_INDEX);      // lane 0 of every workgroup has a sample (j < n)
}

hipError_t afr_launch_dataset_text_w(long long first_seed, const int64_t* seed_rows, const int64_t* out_rows, long long n, int min_len,
                                     int max_len, const uint32_t* cum, int64_t* codes, int ldx, int32_t* len, uint32_t* err, hipStream_t s) {
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(dataset_text_w_kernel, dim3(blocks), dim3(256), 0, s, first_seed, seed_rows, out_rows, n, min_len, max_len, cum, codes, ldx,
                       len, err);
    return hipGetLastError();
}

// A counter pair's mean squared error relative to the reference mean, in 16.16 fixed point: min((((sumsq << 16) / pixels) << 16) / m_ref,
// 16 << 16) without forming q << 16, which need not fit: q / m_ref >= 16 is the cap, else sixteen steps of long division on the
// remainder (< m_ref < 2^63, so its double fits).  pixels != 0, sumsq < 2^47, m_ref >= 1.  Shared by the two weight kernels.
__device__ __forceinline__ unsigned long long text_rel_to_mean(unsigned long long sumsq, unsigned long long pixels, unsigned long long m_ref) {
    const unsigned long long q = (sumsq << 16) / pixels;
    unsigned long long hi = q / m_ref, rem = q - hi * m_ref;
    if (hi >= 16ull) return 16ull << 16;
    for (int b = 0; b < 16; ++b) {
        rem <<= 1; hi <<= 1;
        if (rem >= m_ref) { rem -= m_ref; hi |= 1ull; }
    }
    return hi;
}

// afr_op_text_weights: the table above from afr_op_sheet_char_errors' by-code counters, one workgroup of 128 lanes, lane i = code 33 + i
// (synth.text_weights; the definition is in include/afr.h).  Two 64-bit sums over the members (a tree in LDS), the weight of each member
// in registers, an inclusive scan of the 94 weights in LDS.  No atomics: a second launch stores the same words.
struct TextWeightsArgs {
    const unsigned long long* by_code; uint32_t members[3]; uint32_t floor_w, gain; uint32_t* cum; uint32_t* w;
};
__global__ __launch_bounds__(TXT_PAD) void text_weights_kernel(TextWeightsArgs a) {
    __shared__ unsigned long long s_p[TXT_PAD], s_s[TXT_PAD];
    __shared__ uint32_t s_w[TXT_PAD];
    const int t = threadIdx.x;
    const bool member = t < TXT_CODES && ((a.members[t >> 5] >> (t & 31)) & 1u);
    const bool counted = member && a.by_code && a.gain;                // non-members and the background row are never read
    unsigned long long pixels = counted ? a.by_code[(TXT_FIRST + t) * 5 + 1] : 0ull;
    unsigned long long sumsq = counted ? a.by_code[(TXT_FIRST + t) * 5 + 2] : 0ull;
    s_p[t] = pixels; s_s[t] = sumsq;
    __syncthreads();
    for (int off = TXT_PAD / 2; off > 0; off >>= 1) {
        if (t < off) { s_p[t] += s_p[t + off]; s_s[t] += s_s[t + off]; }
        __syncthreads();
    }
    unsigned long long P = s_p[0], S = s_s[0];
    uint32_t w = member ? a.floor_w : 0u;
    if (member && S != 0ull) {
        const int k = max(0, 64 - __clzll((long long)S) - 47);         // S >> k < 2^47: every << 16 below stays inside 64 bits
        P >>= k; S >>= k; pixels >>= k; sumsq >>= k;
        const unsigned long long m_ref = max(1ull, (S << 16) / max(1ull, P));
        const unsigned long long rel = pixels != 0ull ? text_rel_to_mean(sumsq, pixels, m_ref) : 1ull << 16;
        w = a.floor_w + (uint32_t)(((unsigned long long)a.gain * rel) >> 16);
    }
    s_w[t] = w;
    __syncthreads();
    uint32_t c = w;
    for (int off = 1; off < TXT_PAD; off <<= 1) {
        const uint32_t left = t >= off ? s_w[t - off] : 0u;
        __syncthreads();
        c += left;
        s_w[t] = c;
        __syncthreads();
    }
    if (t < TXT_CODES) {
        a.cum[t] = c;
        if (a.w) a.w[t] = w;
    }
}

hipError_t afr_launch_text_weights(const unsigned long long* by_code, const uint32_t members[3], uint32_t floor_w, uint32_t gain, uint32_t* cum,
                                   uint32_t* w, hipStream_t s) {
    const TextWeightsArgs a{by_code, {members[0], members[1], members[2]}, floor_w, gain, cum, w};
    hipLaunchKernelGGL(text_weights_kernel, dim3(1), dim3(TXT_PAD), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------ Markov text
// afr_op_dataset_text_m: dataset_text_w_kernel with one table row per context (synth.lcg_text_markov): row 0 at the start of a word, row
// 1 + i after letter i.  The 95 rows go to LDS once per workgroup, each padded to 128 entries with 2^32 - 1 (48 640 bytes), so a draw is
// the same seven-step search without a bound check, offset by the context's row.  A sample that reaches a row whose total is 0 stops,
// zero-fills its whole row and flags bit 0 of *err -- one atomic per wave that holds such a sample.
constexpr int TXT_CTX = TXT_CODES + 1;
__global__ __launch_bounds__(256) void dataset_text_m_kernel(long long first_seed, const int64_t* __restrict__ seed_rows,
                                                             const int64_t* __restrict__ out_rows, long long n, int min_len, int max_len,
                                                             const uint32_t* __restrict__ cum2, int64_t* __restrict__ codes, int ldx,
                                                             int32_t* __restrict__ len, uint32_t* __restrict__ err) {
    __shared__ uint32_t s_cum[TXT_CTX * TXT_PAD];
    for (int e = threadIdx.x; e < TXT_CTX * TXT_PAD; e += 256) {
        const int r = e / TXT_PAD, c = e - r * TXT_PAD;
        s_cum[e] = c < TXT_CODES ? cum2[r * TXT_CODES + c] : 0xFFFFFFFFu;
    }
    __syncthreads();
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool failed = false;
    if (j < n) {
        uint32_t state = (uint32_t)(uint64_t)(first_seed + (seed_rows ? seed_rows[j] : j));
        const long long row = out_rows ? out_rows[j] : j;
        int64_t* dst = codes + row * (long long)ldx;
        auto draw = [&](uint32_t k) -> uint32_t {
            state = state * 1664525u + 1013904223u;
            return (uint32_t)(((uint64_t)state * k) >> 32);
        };
        int length = (int)draw((uint32_t)(max_len - min_len + 1)) + min_len, pos = 0;
        int remaining = length;
        while (remaining > 0 && !failed) {
            const int wl = min((int)draw(10u) + 1, remaining);
            const uint32_t* tab = s_cum;                               // a word starts in context 0
            for (int i = 0; i < wl; ++i) {
                const uint32_t total = tab[TXT_CODES - 1];
                if (total == 0u) { failed = true; break; }
                const int at = text_search(tab, draw(total));
                dst[pos++] = TXT_FIRST + at;
                tab = s_cum + (1 + at) * TXT_PAD;                      // at <= 93: r < total = tab[93] ends the search there at the latest
            }
            remaining -= wl;
            if (remaining > 0 && !failed) { dst[pos++] = 32; --remaining; }
        }
        if (failed) length = pos = 0;
        for (; pos < ldx; ++pos) dst[pos] = 0;
        if (len) len[row] = length;
    }
    const unsigned long long any = __ballot(failed);
    if (any && err && (threadIdx.x & 63) == __ffsll((long long)any) - 1) atomicOr(err, AFR_ERR_INDEX);
}

hipError_t afr_launch_dataset_text_m(long long first_seed, const int64_t* seed_rows, const int64_t* out_rows, long long n, int min_len,
                                     int max_len, const uint32_t* cum2, int64_t* codes, int ldx, int32_t* len, uint32_t* err, hipStream_t s) {
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(dataset_text_m_kernel, dim3(blocks), dim3(256), 0, s, first_seed, seed_rows, out_rows, n, min_len, max_len, cum2, codes, ldx,
                       len, err);
    return hipGetLastError();
}

// afr_op_pair_errors: the table is 95 x 94 x 4 counters of 8 bytes, 285 760 bytes, so no workgroup can hold it in LDS whole.  The grid is
// (chunks of samples) x (8 bands of 12 contexts): a workgroup keeps its band's 12 x 94 x 4 64-bit counters in LDS (36 096 bytes), walks
// the positions of its chunk -- a lane reads its code and the code before it, and only when the context falls into the band and the
// position contributes its record of per_pos, adding {1, pixels, sumsq, wrong} with LDS atomics -- and at the end adds every non-zero
// counter to by_pair with one 64-bit global atomic.  Each band reads the codes once more (8 bytes a position) but every record is read
// by one band only.  The host sizes the chunks for about 64 of them, 16 samples at the least: one global atomic then stands for the
// adds of some hundreds of sheets.  Against one lane per position adding straight to by_pair (four global atomics per contribution,
// a few hundred hot addresses) this form was measured several times faster at 30 000 sheets; profiles/pairs/ has both.
constexpr int PAIR_BANDS = 8, PAIR_BAND_ROWS = 12, PAIR_BAND_WORDS = PAIR_BAND_ROWS * TXT_CODES * 4;
static_assert(PAIR_BANDS * PAIR_BAND_ROWS >= TXT_CTX, "the bands cover every context");
__global__ __launch_bounds__(256) void pair_errors_kernel(const int64_t* __restrict__ codes, int ldx, const int64_t* __restrict__ code_rows,
                                                          long long n, long long chunk, const uint32_t* __restrict__ per_pos,
                                                          unsigned long long* __restrict__ by_pair) {
    __shared__ unsigned long long s_by[PAIR_BAND_WORDS];
    const int t = threadIdx.x, lo = blockIdx.y * PAIR_BAND_ROWS;
    for (int e = t; e < PAIR_BAND_WORDS; e += 256) s_by[e] = 0ull;
    __syncthreads();
    const long long j0 = (long long)blockIdx.x * chunk, j1 = min(n, j0 + chunk);
    for (long long e = j0 * ldx + t; e < j1 * ldx; e += 256) {
        const long long j = e / ldx;
        const int i = (int)(e - j * ldx);
        const int64_t* src = codes + (code_rows ? code_rows[j] : j) * (long long)ldx;
        const long long c = src[i];
        if (c < TXT_FIRST || c >= TXT_FIRST + TXT_CODES) continue;
        const long long p = i > 0 ? src[i - 1] : 0;
        const int r = (p >= TXT_FIRST && p < TXT_FIRST + TXT_CODES ? 1 + (int)(p - TXT_FIRST) : 0) - lo;
        if ((unsigned)r >= (unsigned)PAIR_BAND_ROWS) continue;
        const uint4 rec = ((const uint4*)per_pos)[(size_t)j * (size_t)(ldx + 1) + i];      // {pixels, sumsq, off2, wrong}
        if (rec.x == 0u) continue;
        unsigned long long* dst = s_by + (r * TXT_CODES + (int)(c - TXT_FIRST)) * 4;
        atomicAdd(dst, 1ull);
        atomicAdd(dst + 1, (unsigned long long)rec.x);
        if (rec.y) atomicAdd(dst + 2, (unsigned long long)rec.y);
        if (rec.w) atomicAdd(dst + 3, (unsigned long long)rec.w);
    }
    __syncthreads();
    const int words = min(PAIR_BAND_WORDS, (TXT_CTX - lo) * TXT_CODES * 4);                // the last band ends with the table
    for (int e = t; e < words; e += 256)
        if (s_by[e]) atomicAdd(by_pair + (size_t)lo * TXT_CODES * 4 + e, s_by[e]);
}

hipError_t afr_launch_pair_errors(const int64_t* codes, int ldx, const int64_t* code_rows, long long n, const uint32_t* per_pos,
                                  unsigned long long* by_pair, hipStream_t s) {
    const long long chunk = max(16ll, (n + 63) / 64);
    const unsigned chunks = (unsigned)((n + chunk - 1) / chunk);
    hipLaunchKernelGGL(pair_errors_kernel, dim3(chunks, PAIR_BANDS), dim3(256), 0, s, codes, ldx, code_rows, n, chunk, per_pos, by_pair);
    return hipGetLastError();
}

// afr_op_pair_weights: the Markov table from the pair counters, one workgroup of 256 lanes (synth.pair_weights; the definition is in
// include/afr.h).  The lanes stride over the 95 x 94 pairs twice: once for the two 64-bit sums over the live pairs (a tree in LDS), once
// for each pair's weight, kept in LDS; lane r < 95 then sums row r in order and stores its cumulative weights.  A record that is not
// live is never read.  No atomics: a second launch stores the same words.
struct PairWeightsArgs {
    const unsigned long long* by_pair; uint32_t members[3]; uint32_t floor_w, gain, min_chars; uint32_t* cum2; uint32_t* w2;
};
__device__ __forceinline__ bool text_member(const uint32_t m[3], int i) {
    return ((i < 32 ? m[0] : i < 64 ? m[1] : m[2]) >> (i & 31)) & 1u;
}
__global__ __launch_bounds__(256) void pair_weights_kernel(PairWeightsArgs a) {
    __shared__ unsigned long long s_p[256], s_s[256];
    __shared__ uint32_t s_w[TXT_CTX * TXT_CODES];
    const int t = threadIdx.x;
    const bool counted = a.by_pair && a.gain;
    auto live = [&](int e) -> bool {
        const int r = e / TXT_CODES, c = e - r * TXT_CODES;
        return text_member(a.members, c) && (r == 0 || text_member(a.members, r - 1));
    };
    unsigned long long P = 0ull, S = 0ull;
    if (counted)
        for (int e = t; e < TXT_CTX * TXT_CODES; e += 256)
            if (live(e)) { P += a.by_pair[e * 4 + 1]; S += a.by_pair[e * 4 + 2]; }
    s_p[t] = P; s_s[t] = S;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) { s_p[t] += s_p[t + off]; s_s[t] += s_s[t + off]; }
        __syncthreads();
    }
    P = s_p[0]; S = s_s[0];
    const int k = S ? max(0, 64 - __clzll((long long)S) - 47) : 0;     // S >> k < 2^47: every << 16 below stays inside 64 bits
    const unsigned long long m_ref = max(1ull, ((S >> k) << 16) / max(1ull, P >> k));
    for (int e = t; e < TXT_CTX * TXT_CODES; e += 256) {
        uint32_t w = 0u;
        if (live(e)) {
            unsigned long long rel = 1ull << 16;
            if (S != 0ull) {
                const unsigned long long chars = a.by_pair[e * 4], pixels = a.by_pair[e * 4 + 1] >> k, sumsq = a.by_pair[e * 4 + 2] >> k;
                if (pixels != 0ull && chars >= a.min_chars) rel = text_rel_to_mean(sumsq, pixels, m_ref);
            }
            w = S != 0ull ? a.floor_w + (uint32_t)(((unsigned long long)a.gain * rel) >> 16) : a.floor_w;
        }
        s_w[e] = w;
        if (a.w2) a.w2[e] = w;
    }
    __syncthreads();
    if (t < TXT_CTX) {
        uint32_t c = 0u;
        for (int i = 0; i < TXT_CODES; ++i) {
            c += s_w[t * TXT_CODES + i];
            a.cum2[t * TXT_CODES + i] = c;
        }
    }
}

hipError_t afr_launch_pair_weights(const unsigned long long* by_pair, const uint32_t members[3], uint32_t floor_w, uint32_t gain,
                                   uint32_t min_chars, uint32_t* cum2, uint32_t* w2, hipStream_t s) {
    const PairWeightsArgs a{by_pair, {members[0], members[1], members[2]}, floor_w, gain, min_chars, cum2, w2};
    hipLaunchKernelGGL(pair_weights_kernel, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------- compose
// One workgroup of 256 threads per sheet, grid-stride.  The atlas's cells are copied into LDS once per workgroup (the paint phase
// gathers single bytes from them at per-lane addresses, which LDS serves and a global load does not); advances and kerning are read
// once per character from global memory (L2 resident).  Per sheet:
//   text    lane t holds code t; the text ends at the first 0 (ballot), codes outside the atlas are dropped and flagged, the rest is
//           packed in order (ballot + popcount prefix);
//   layout  lane t fetches its character's advance and its kerning against the character before it; ONE lane then walks the text
//           (<= 256 characters, LDS only) and restates datagen.wrap_text over prefix sums: a line is always a contiguous piece of
//           the text, [ls, le), so width64(line + " " + word) is a difference of two prefix sums less the kerning into the line's
//           first character; lane t then turns its character's pen into a pixel, (pen64 + 32) >> 6;
//   index   lane e of n_lines * width / 8 scans one line once for the first and the last glyph whose cell overlaps one 8-pixel column
//           block (pens need not be monotonic under kerning, so this is a range to scan, not the set);
//   paint   output driven: a lane owns 8 consecutive pixels, starts them at coverage 0, composites every glyph of that range whose
//           cell covers them in (line, character) order and stores the 8 bytes once.
struct ComposeLds {
    int code[CMP_MAX_LDX + 1], adv[CMP_MAX_LDX + 1], kern[CMP_MAX_LDX + 1], S[CMP_MAX_LDX + 1], px[CMP_MAX_LDX + 1];
    int ls[CMP_MAX_LINES], le[CMP_MAX_LINES], base[CMP_MAX_LINES];
    int wave_zero[4], wave_count[4];
    int n_lines;
};
size_t afr_compose_static_lds() { return sizeof(ComposeLds); }
// dynamic LDS: the cells, padded to whole words, then one (first, last) pair of shorts per line and 8-pixel column block
static __host__ __device__ inline size_t compose_cell_lds(int n_codes, int cell_h, int cell_w) { return ((size_t)n_codes * cell_h * cell_w + 3) & ~(size_t)3; }
size_t afr_compose_dynamic_lds(int n_codes, int cell_h, int cell_w, int n_lines, int width) {
    return compose_cell_lds(n_codes, cell_h, cell_w) + (size_t)n_lines * (width / 8) * sizeof(short2);
}

// The text, layout and index phases of one sheet, for the 256 threads of a workgroup: row `row` of a.codes is read, packed into L.code
// (and, with POS, every packed character's index in its row into s_pos), wrapped and penned, and s_range filled.  Returns the number of
// lines drawn; `placed` is whether lane t's packed character stands on one of them.  Ends behind a barrier.
template <bool POS>
__device__ __forceinline__ int sheet_layout(const ComposeArgs& a, ComposeLds& L, int* s_pos, short2* s_range, long long row, int t, int lane,
                                            int wave, int W8, bool& placed) {
    // ---- text
    const long long c = t < a.ldx ? a.codes[row * a.ldx + t] : 0;
    const unsigned long long zeros = __ballot(c == 0);
    if (lane == 0) L.wave_zero[wave] = zeros ? wave * 64 + __ffsll((long long)zeros) - 1 : CMP_MAX_LDX;
    __syncthreads();
    const int len = min(min(L.wave_zero[0], L.wave_zero[1]), min(L.wave_zero[2], L.wave_zero[3]));
    const bool in_range = c >= 0 && c < a.n_codes;
    const bool valid = t < len && in_range;
    const unsigned long long keep = __ballot(valid), bad = __ballot(t < len && !in_range);
    if (lane == 0) {
        L.wave_count[wave] = __popcll(keep);
        if (bad && a.err) atomicOr(a.err, AFR_ERR_INDEX);
    }
    __syncthreads();
    int before = 0, n_txt = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) before += L.wave_count[w];
        n_txt += L.wave_count[w];
    }
    if (valid) {
        const int g = before + __popcll(keep & ((1ull << lane) - 1ull));
        L.code[g] = (int)c;
        if (POS) s_pos[g] = t;
    }
    __syncthreads();
    // ---- layout
    if (t < n_txt) {
        const int cc = L.code[t];
        L.adv[t] = a.adv64[cc];
        L.kern[t] = t > 0 && a.kern64 ? (int)a.kern64[(size_t)L.code[t - 1] * a.n_codes + cc] : 0;
    }
    __syncthreads();
    if (t == 0) {
        // S = width of text[0, pos) with every kerning; width64(text[s, e)) = S[e] - S[s] - kern[s] for e > s.
        // current = text[ls, le); the word being read starts at ws.
        int S = 0, ls = 0, le = 0, S_ls = 0, ws = 0, S_ws = 0, nl = 0;
        for (int pos = 0; pos <= n_txt && nl < a.n_lines; ++pos) {
            L.S[pos] = S;
            const bool end = pos == n_txt;
            const int step = end ? 0 : L.adv[pos] + L.kern[pos];
            if (end || L.code[pos] == 32) {
                const bool cur = le > ls;
                const int cs = cur ? ls : ws, S_cs = cur ? S_ls : S_ws;
                const int width = pos > cs ? S - S_cs - L.kern[cs] : 0;
                if (width > a.wrap_width64 && cur) {
                    L.ls[nl] = ls; L.le[nl] = le; ++nl;            // emit current; current = word
                    ls = ws; S_ls = S_ws;
                } else {
                    ls = cs; S_ls = S_cs;                          // current = candidate
                }
                le = pos;
                ws = pos + 1; S_ws = S + step;
            }
            S += step;
        }
        if (nl < a.n_lines && le > ls) { L.ls[nl] = ls; L.le[nl] = le; ++nl; }
        L.n_lines = nl;
    }
    __syncthreads();
    const int nl = L.n_lines;
    placed = false;
    if (t < n_txt) {
        for (int i = 0; i < nl; ++i) {
            const int ls = L.ls[i];
            if (t >= ls && t < L.le[i]) {
                const int pen64 = L.S[t] + L.kern[t] - L.S[ls] - L.kern[ls];      // 0 for the line's first character
                L.px[t] = (pen64 + 32) >> 6;
                placed = true;
            }
        }
    }
    __syncthreads();
    // ---- index
    for (int e = t; e < nl * W8; e += 256) {
        const int i = e / W8, x0 = (e - i * W8) << 3, le = L.le[i];
        int first = le, last = L.ls[i] - 1;
        for (int g = L.ls[i]; g < le; ++g) {
            const int rx0 = x0 - L.px[g] + a.origin_x;
            if (rx0 > -8 && rx0 < a.cell_w) { first = min(first, g); last = g; }
        }
        s_range[e] = make_short2((short)first, (short)last);
    }
    __syncthreads();
    return nl;
}

// the atlas's cells (and the baselines) into LDS, once per workgroup
__device__ __forceinline__ void sheet_cells_to_lds(const ComposeArgs& a, ComposeLds& L, uint8_t* s_cells, int t) {
    const int cell_bytes = a.n_codes * a.cell_h * a.cell_w;
    const uint32_t* src = (const uint32_t*)a.cells;                    // 4-byte aligned (checked by the caller)
    uint32_t* dst = (uint32_t*)s_cells;
    for (int i = t; i < cell_bytes / 4; i += 256) dst[i] = src[i];
    for (int i = (cell_bytes & ~3) + t; i < cell_bytes; i += 256) s_cells[i] = a.cells[i];
    if (t < CMP_MAX_LINES) L.base[t] = a.baseline[t];
}

__global__ __launch_bounds__(256) void compose_sheets_kernel(ComposeArgs a) {
    extern __shared__ __align__(16) uint8_t s_cells[];                 // [n_codes][cell_h][cell_w], padded to whole words
    __shared__ ComposeLds L;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    sheet_cells_to_lds(a, L, s_cells, t);
    const int W8 = a.width >> 3, chunks = a.height * W8;
    short2* s_range = (short2*)(s_cells + compose_cell_lds(a.n_codes, a.cell_h, a.cell_w));      // [n_lines][W8]
    for (long long j = blockIdx.x; j < a.n; j += gridDim.x) {
        __syncthreads();                                               // the cells are in; the sheet before this one is painted
        bool placed;
        const int nl = sheet_layout<false>(a, L, nullptr, s_range, j, t, lane, wave, W8, placed);
        // ---- paint
        uint8_t* dst = a.out + (size_t)(a.out_rows ? a.out_rows[j] : j) * (size_t)chunks * 8u;
        for (int q = t; q < chunks; q += 256) {
            const int y = q / W8, x0 = (q - y * W8) << 3;
            unsigned m[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
            for (int i = 0; i < nl; ++i) {
                const int ry = y - L.base[i] + a.origin_y;
                if ((unsigned)ry >= (unsigned)a.cell_h) continue;
                const short2 range = s_range[i * W8 + (x0 >> 3)];
                for (int g = range.x; g <= range.y; ++g) {
                    const int rx0 = x0 - L.px[g] + a.origin_x;         // the cell column under the chunk's first pixel
                    if (rx0 <= -8 || rx0 >= a.cell_w) continue;
                    const uint8_t* row = s_cells + (L.code[g] * a.cell_h + ry) * a.cell_w;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int rx = rx0 + k;
                        if ((unsigned)rx < (unsigned)a.cell_w) {
                            const unsigned b = row[rx];
                            m[k] = m[k] + b - (m[k] * b + 127u) / 255u;
                        }
                    }
                }
            }
            uint2 v;
            v.x = (255u - m[0]) | (255u - m[1]) << 8 | (255u - m[2]) << 16 | (255u - m[3]) << 24;
            v.y = (255u - m[4]) | (255u - m[5]) << 8 | (255u - m[6]) << 16 | (255u - m[7]) << 24;
            *(uint2*)(dst + (size_t)q * 8u) = v;
        }
    }
}

// ------------------------------------------------------------------------------------ char errors
// afr_op_sheet_char_errors: compose's text, layout and index phases over the same LDS, then a paint phase that loads where compose
// stores.  A lane recomputes the coverage m of its 8 pixels (the target is 255 - m, never read) and remembers per pixel the glyph with
// the largest cell value b > 0, the earlier one on a tie: the pixel's owner.  The 8 prediction bytes come in one load.  Pixels without
// an owner are summed in registers and across the wave; owned pixels go to the owner's record in LDS, indexed by the character's
// position in its row of codes, one integer add per field and run of pixels with the same owner.  After the sheet the records are
// added by code into 64-bit LDS counters that live as long as the workgroup (a 32-bit sumsq holds one sheet, not several), stored
// once to per_pos and cleared; the counters go to by_code at the end, one global atomic per non-zero field.
struct CharErrLds {
    int pos[CMP_MAX_LDX + 1];
    __align__(16) uint32_t acc[CMP_MAX_LDX + 1][4];                    // {pixels, sumsq, off2, wrong} by position; slot ldx = background
};
size_t afr_charerr_static_lds() { return sizeof(ComposeLds) + sizeof(CharErrLds); }
static __host__ __device__ inline size_t charerr_by_lds(int n_codes) { return (size_t)(n_codes + 1) * 5 * sizeof(unsigned long long); }
size_t afr_charerr_dynamic_lds(int n_codes, int cell_h, int cell_w, int n_lines, int width) {
    return charerr_by_lds(n_codes) + afr_compose_dynamic_lds(n_codes, cell_h, cell_w, n_lines, width);
}

__device__ __forceinline__ void charerr_add(uint32_t* rec, uint32_t pixels, uint32_t sumsq, uint32_t off2, uint32_t wrong) {
    atomicAdd(&rec[0], pixels);
    if (sumsq) atomicAdd(&rec[1], sumsq);
    if (off2) atomicAdd(&rec[2], off2);
    if (wrong) atomicAdd(&rec[3], wrong);
}

// one character (or one sheet's background) and its record into the workgroup's counters of its code
__device__ __forceinline__ void charerr_by_code(unsigned long long* by, const uint32_t* rec) {
    atomicAdd(&by[0], 1ull);
#pragma unroll
    for (int f = 0; f < 4; ++f)
        if (rec[f]) atomicAdd(&by[1 + f], (unsigned long long)rec[f]);
}

__global__ __launch_bounds__(256) void sheet_char_errors_kernel(CharErrArgs ca) {
    extern __shared__ __align__(16) uint8_t s_dyn[];                   // the by-code counters, then compose's cells and ranges
    __shared__ ComposeLds L;
    __shared__ CharErrLds X;
    const ComposeArgs& a = ca.c;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned long long* s_by = (unsigned long long*)s_dyn;             // [n_codes + 1][5]
    uint8_t* s_cells = s_dyn + charerr_by_lds(a.n_codes);
    const int n_by = (a.n_codes + 1) * 5;
    sheet_cells_to_lds(a, L, s_cells, t);
    for (int e = t; e < n_by; e += 256) s_by[e] = 0ull;
    for (int e = t; e < (CMP_MAX_LDX + 1) * 4; e += 256) (&X.acc[0][0])[e] = 0u;
    const int W8 = a.width >> 3, chunks = a.height * W8;
    short2* s_range = (short2*)(s_cells + compose_cell_lds(a.n_codes, a.cell_h, a.cell_w));      // [n_lines][W8]
    for (long long j = blockIdx.x; j < a.n; j += gridDim.x) {
        __syncthreads();                                               // LDS is set up; the sheet before this one is stored and cleared
        bool placed;
        const int nl = sheet_layout<true>(a, L, X.pos, s_range, a.out_rows ? a.out_rows[j] : j, t, lane, wave, W8, placed);
        // ---- measure
        const uint8_t* src = ca.pred + (size_t)j * (size_t)chunks * 8u;
        uint32_t bg[4] = {0u, 0u, 0u, 0u};
        for (int q = t; q < chunks; q += 256) {
            const int y = q / W8, x0 = (q - y * W8) << 3;
            unsigned m[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, top[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
            int own[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int i = 0; i < nl; ++i) {
                const int ry = y - L.base[i] + a.origin_y;
                if ((unsigned)ry >= (unsigned)a.cell_h) continue;
                const short2 range = s_range[i * W8 + (x0 >> 3)];
                for (int g = range.x; g <= range.y; ++g) {
                    const int rx0 = x0 - L.px[g] + a.origin_x;
                    if (rx0 <= -8 || rx0 >= a.cell_w) continue;
                    const uint8_t* row = s_cells + (L.code[g] * a.cell_h + ry) * a.cell_w;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int rx = rx0 + k;
                        if ((unsigned)rx < (unsigned)a.cell_w) {
                            const unsigned b = row[rx];
                            m[k] = m[k] + b - (m[k] * b + 127u) / 255u;
                            if (b > top[k]) { top[k] = b; own[k] = g; }      // strictly larger: the earlier glyph keeps a tie
                        }
                    }
                }
            }
            const uint2 v = *(const uint2*)(src + (size_t)q * 8u);
            int run = -1;
            uint32_t r[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int p = (int)(((k < 4 ? v.x : v.y) >> (8 * (k & 3))) & 255u), tl = 255 - (int)m[k];
                const uint32_t d = (uint32_t)abs(p - tl);
                const uint32_t sq = d * d, o2 = d >= 2u, wr = (p >= 128) != (tl >= 128);
                if (top[k] == 0u) {
                    bg[0] += 1u; bg[1] += sq; bg[2] += o2; bg[3] += wr;
                } else {
                    if (own[k] != run) {
                        if (run >= 0) charerr_add(X.acc[X.pos[run]], r[0], r[1], r[2], r[3]);
                        run = own[k];
                        r[0] = r[1] = r[2] = r[3] = 0u;
                    }
                    r[0] += 1u; r[1] += sq; r[2] += o2; r[3] += wr;
                }
            }
            if (run >= 0) charerr_add(X.acc[X.pos[run]], r[0], r[1], r[2], r[3]);
        }
#pragma unroll
        for (int f = 0; f < 4; ++f) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) bg[f] += __shfl_xor(bg[f], off);
            if (lane == 0 && bg[f]) atomicAdd(&X.acc[a.ldx][f], bg[f]);
        }
        __syncthreads();
        // ---- by code: every character placed on a drawn line, and the background
        if (ca.by_code) {
            if (placed) charerr_by_code(s_by + L.code[t] * 5, X.acc[X.pos[t]]);
            if (t == 0) charerr_by_code(s_by + a.n_codes * 5, X.acc[a.ldx]);
        }
        __syncthreads();
        // ---- per position: every record of row j stored once, and cleared for the next sheet
        for (int e = t; e <= a.ldx; e += 256) {
            uint4* rec = (uint4*)X.acc[e];
            if (ca.per_pos) ((uint4*)ca.per_pos)[(size_t)j * (size_t)(a.ldx + 1) + e] = *rec;
            *rec = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    __syncthreads();
    if (ca.by_code)
        for (int e = t; e < n_by; e += 256)
            if (s_by[e]) atomicAdd(ca.by_code + e, s_by[e]);
}

// -------------------------------------------------------------------------------------- read back
// afr_op_sheet_read_back: compose's text, layout and index phases over the same LDS, then one WAVE per scored character (a character
// on a drawn line, not a space, whose cell box clipped to the sheet -- its window -- is not empty), the characters dealt to the four
// waves in turn.  Per character:
//   stage   lane = window pixel: a = 255 - pred and ctx = compose's fold over every OTHER glyph that covers the pixel (the paint
//           phase's loop over the lines and s_range, the scored glyph skipped) go to the wave's own LDS row as one halfword a | ctx << 8;
//   score   lane = candidate.  The 96 slots are the codes 32..126 (slot 0, the blank, always; a slot 1 + i if member bit i is set or
//           the code is the character's own) and slot 95 = the character's own code when it lies outside 32..126; a lane holds slots
//           lane and lane + 64.  It walks the window once: the halfword is one broadcast read, the two cells' bytes are read at
//           per-lane addresses; the two sums of (a - hyp)^2 stay in registers.  No reduction per candidate;
//   pick    one 64-bit min over the wave of score << 32 | rank, rank 0 for the character's own code and code + 1 otherwise: the
//           smallest score, the true code first among equals, then the smallest code.
// The winner and the two scores go to records by position in LDS, stored once per row after the sheet's barrier and cleared.  The
// confusion counts of the true codes 33..126 live in LDS for as long as the workgroup does, as 16-bit counters packed in pairs (a
// 32-bit table beside Montserrat's cells would pass the LDS budget): a sheet adds at most ldx, so the table is added to global memory
// -- one 64-bit atomic per non-zero counter -- whenever the next sheet could carry a counter past 65535, and at the end.  A true code
// outside 33..126 (nothing the text sources draw) adds straight to global memory.
constexpr int RB_SLOTS = 96, RB_CONF_WORDS = TXT_CODES * RB_SLOTS / 2, RB_CONF_MAX = 65535;
struct ReadBackLds {
    int pos[CMP_MAX_LDX + 1], line[CMP_MAX_LDX];
    uint32_t rd[CMP_MAX_LDX];
    __align__(8) uint2 sc[CMP_MAX_LDX];                                // {winner's score, score of the true code} by position
};
size_t afr_readback_static_lds() { return sizeof(ComposeLds) + sizeof(ReadBackLds); }
static __host__ __device__ inline size_t readback_stage_lds(int cell_h, int cell_w) { return ((size_t)cell_h * cell_w * 2 + 3) & ~(size_t)3; }
size_t afr_readback_dynamic_lds(int n_codes, int cell_h, int cell_w, int n_lines, int width) {
    return (size_t)RB_CONF_WORDS * 4 + 4 * readback_stage_lds(cell_h, cell_w) + afr_compose_dynamic_lds(n_codes, cell_h, cell_w, n_lines, width);
}

// the workgroup's confusion counters added to global memory and cleared; a thread owns its words, so no barrier in between
__device__ __forceinline__ void readback_flush(uint32_t* s_conf, unsigned long long* confusion, int n_codes, int t) {
    for (int w = t; w < RB_CONF_WORDS; w += 256) {
        const uint32_t v = s_conf[w];
        if (!v) continue;
        s_conf[w] = 0u;
        const int e = 2 * w, r = e / RB_SLOTS, col = e - r * RB_SLOTS;      // RB_SLOTS is even: both halves lie in row r
        unsigned long long* dst = confusion + (size_t)(TXT_FIRST + r) * n_codes + 32 + col;
        if (v & 0xFFFFu) atomicAdd(dst, (unsigned long long)(v & 0xFFFFu));
        if (v >> 16) atomicAdd(dst + 1, (unsigned long long)(v >> 16));
    }
}

// bit i of the 94-bit mask (false outside it), without indexing the kernel argument by a register
__device__ __forceinline__ bool readback_member(const uint32_t m[3], int i) {
    if (i < 0 || i >= TXT_CODES) return false;
    return ((i < 32 ? m[0] : i < 64 ? m[1] : m[2]) >> (i & 31)) & 1u;
}

// LDS written by some lanes of a wave is read by others of the same wave
__device__ __forceinline__ void readback_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ __launch_bounds__(256) void sheet_read_back_kernel(ReadBackArgs ra) {
    extern __shared__ __align__(16) uint8_t s_dyn[];                   // the confusion counters, the waves' windows, compose's cells and ranges
    __shared__ ComposeLds L;
    __shared__ ReadBackLds R;
    const ComposeArgs& a = ra.c;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t* s_conf = (uint32_t*)s_dyn;                               // [94][96] uint16, two to a word
    const size_t stage = readback_stage_lds(a.cell_h, a.cell_w);
    uint16_t* s_win = (uint16_t*)(s_dyn + (size_t)RB_CONF_WORDS * 4 + (size_t)wave * stage);
    uint8_t* s_cells = s_dyn + (size_t)RB_CONF_WORDS * 4 + 4 * stage;
    sheet_cells_to_lds(a, L, s_cells, t);
    for (int e = t; e < RB_CONF_WORDS; e += 256) s_conf[e] = 0u;
    R.rd[t] = 0u;
    R.sc[t] = make_uint2(0u, 0u);
    const int W8 = a.width >> 3, cell_px = a.cell_h * a.cell_w;
    short2* s_range = (short2*)(s_cells + compose_cell_lds(a.n_codes, a.cell_h, a.cell_w));      // [n_lines][W8]
    // this lane's two slots: whether the mask admits them, and their codes (slot 95 and a closed slot read the blank's cell, unused)
    const int slot1 = lane + 64;
    const bool open0 = lane == 0 || readback_member(ra.members, lane - 1);
    const bool open1 = readback_member(ra.members, slot1 - 1);
    int since = 0;                                                     // an upper bound of the largest counter in s_conf
    for (long long j = blockIdx.x; j < a.n; j += gridDim.x) {
        __syncthreads();                                               // LDS is set up; the sheet before this one is stored and cleared
        if (ra.confusion && since + a.ldx > RB_CONF_MAX) {
            readback_flush(s_conf, ra.confusion, a.n_codes, t);
            since = 0;
        }
        since += a.ldx;
        bool placed;
        const int nl = sheet_layout<true>(a, L, R.pos, s_range, a.out_rows ? a.out_rows[j] : j, t, lane, wave, W8, placed);
        int my_line = -1;
        if (placed)
            for (int i = 0; i < nl; ++i)
                if (t >= L.ls[i] && t < L.le[i]) my_line = i;
        R.line[t] = my_line;
        __syncthreads();
        // ---- score: wave `wave` takes the characters wave, wave + 4, ... up to the end of the last drawn line
        const uint8_t* src = ra.pred + (size_t)j * (size_t)a.height * (size_t)a.width;
        const int n_end = nl ? L.le[nl - 1] : 0;
        for (int g = wave; g < n_end; g += 4) {
            const int i = R.line[g], c = L.code[g];
            if (i < 0 || c == 32) continue;
            const int top = L.base[i] - a.origin_y, left = L.px[g] - a.origin_x;
            const int y0 = max(top, 0), y1 = min(top + a.cell_h, a.height), x0 = max(left, 0), x1 = min(left + a.cell_w, a.width);
            if (y0 >= y1 || x0 >= x1) continue;
            const int ww = x1 - x0, np = ww * (y1 - y0);
            // ---- stage
            for (int p = lane; p < np; p += 64) {
                const int wy = p / ww, y = y0 + wy, x = x0 + (p - wy * ww);
                unsigned m = 0u;
                for (int l = 0; l < nl; ++l) {
                    const int ry = y - L.base[l] + a.origin_y;
                    if ((unsigned)ry >= (unsigned)a.cell_h) continue;
                    const short2 range = s_range[l * W8 + (x >> 3)];
                    for (int o = range.x; o <= range.y; ++o) {
                        const int rx = x - L.px[o] + a.origin_x;
                        if (o == g || (unsigned)rx >= (unsigned)a.cell_w) continue;
                        const unsigned b = s_cells[(L.code[o] * a.cell_h + ry) * a.cell_w + rx];
                        m = m + b - (m * b + 127u) / 255u;
                    }
                }
                s_win[p] = (uint16_t)((255u - src[(size_t)y * a.width + x]) | m << 8);
            }
            readback_wave_sync();
            // ---- the lane's two candidates over the window
            const bool own_far = c < 32 || c > 126;                    // the character's own code has no slot among 32..126: slot 95
            const int k0 = 32 + lane, k1 = slot1 < RB_SLOTS - 1 ? 32 + slot1 : (own_far ? c : 32);
            const bool use0 = open0 || k0 == c, use1 = open1 || k1 == c;
            const uint8_t* cell0 = s_cells + k0 * cell_px + (y0 - top) * a.cell_w + (x0 - left);
            const uint8_t* cell1 = s_cells + k1 * cell_px + (y0 - top) * a.cell_w + (x0 - left);
            uint32_t s0 = 0u, s1 = 0u;
            // eight pixels of a row at a time: their 24 LDS reads are issued together (the loop is bound by LDS latency, not by
            // arithmetic), a row's last group re-reads the row's last pixel in the lanes' unused places and leaves it out of the sums
            const uint16_t* win = s_win;
            for (int wy = 0; wy < y1 - y0; ++wy, cell0 += a.cell_w, cell1 += a.cell_w, win += ww) {
                for (int wx = 0; wx < ww; wx += 8) {
                    unsigned v[8], b0[8], b1[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int x = min(wx + k, ww - 1);
                        v[k] = win[x]; b0[k] = cell0[x]; b1[k] = cell1[x];
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        if (wx + k >= ww) break;
                        const unsigned av = v[k] & 255u, m = v[k] >> 8;
                        const int d0 = (int)av - (int)(m + b0[k] - (m * b0[k] + 127u) / 255u);
                        const int d1 = (int)av - (int)(m + b1[k] - (m * b1[k] + 127u) / 255u);
                        s0 += (uint32_t)(d0 * d0);
                        s1 += (uint32_t)(d1 * d1);
                    }
                }
            }
            // ---- pick
            const unsigned long long none = ~0ull;
            const unsigned long long key0 = use0 ? (unsigned long long)s0 << 32 | (uint32_t)(k0 == c ? 0 : k0 + 1) : none;
            const unsigned long long key1 = use1 ? (unsigned long long)s1 << 32 | (uint32_t)(k1 == c ? 0 : k1 + 1) : none;
            unsigned long long best = key0 < key1 ? key0 : key1;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long other = __shfl_xor(best, off);
                best = other < best ? other : best;
            }
            const int pos = R.pos[g];
            if (k0 == c) R.sc[pos].y = s0;
            if (k1 == c && use1) R.sc[pos].y = s1;
            if (lane == 0) {
                const int rank = (int)(uint32_t)best, rd = rank ? rank - 1 : c;
                R.rd[pos] = (uint32_t)rd;
                R.sc[pos].x = (uint32_t)(best >> 32);
                if (ra.confusion) {
                    if (c >= TXT_FIRST && c < TXT_FIRST + TXT_CODES) {  // then rd is one of 32..126
                        const int e = (c - TXT_FIRST) * RB_SLOTS + rd - 32;
                        atomicAdd(&s_conf[e >> 1], 1u << (16 * (e & 1)));
                    } else {
                        atomicAdd(ra.confusion + (size_t)c * a.n_codes + rd, 1ull);
                    }
                }
            }
            readback_wave_sync();                                      // the window is read before the next character's is staged
        }
        __syncthreads();
        // ---- every element of row j stored once, and the records cleared for the next sheet
        if (t < a.ldx) {
            if (ra.read) ra.read[(size_t)j * a.ldx + t] = (uint8_t)R.rd[t];
            if (ra.score) ((uint2*)ra.score)[(size_t)j * a.ldx + t] = R.sc[t];
            R.rd[t] = 0u;
            R.sc[t] = make_uint2(0u, 0u);
        }
    }
    __syncthreads();
    if (ra.confusion) readback_flush(s_conf, ra.confusion, a.n_codes, t);
}

int afr_compose_blocks(long long n) { return (int)(n < AFR_COMPOSE_MAX_BLOCKS ? n : AFR_COMPOSE_MAX_BLOCKS); }

hipError_t afr_launch_compose_sheets(const ComposeArgs& a, hipStream_t s) {
    const size_t lds = afr_compose_dynamic_lds(a.n_codes, a.cell_h, a.cell_w, a.n_lines, a.width);
    hipLaunchKernelGGL(compose_sheets_kernel, dim3(afr_compose_blocks(a.n)), dim3(256), lds, s, a);
    return hipGetLastError();
}

hipError_t afr_launch_sheet_char_errors(const CharErrArgs& ca, hipStream_t s) {
    const ComposeArgs& a = ca.c;
    const size_t lds = afr_charerr_dynamic_lds(a.n_codes, a.cell_h, a.cell_w, a.n_lines, a.width);
    hipLaunchKernelGGL(sheet_char_errors_kernel, dim3(afr_compose_blocks(a.n)), dim3(256), lds, s, ca);
    return hipGetLastError();
}

hipError_t afr_launch_sheet_read_back(const ReadBackArgs& ra, hipStream_t s) {
    const ComposeArgs& a = ra.c;
    const size_t lds = afr_readback_dynamic_lds(a.n_codes, a.cell_h, a.cell_w, a.n_lines, a.width);
    hipLaunchKernelGGL(sheet_read_back_kernel, dim3(afr_compose_blocks(a.n)), dim3(256), lds, s, ra);
    return hipGetLastError();
}
