// afr_api.hip -- the C ABI of libafr.so (include/afr.h): plan construction, workspace carve-up and the
// launch sequences of forward / loss / backward / AdamW for both model families.
#include "afr_common.h"
#include "../../include/afr.h"
static_assert(AFR_LOSS_MSE == LOSS_MSE && AFR_LOSS_BCE == LOSS_BCE, "afr.h and afr_common.h name the same loss kinds");

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

// --------------------------------------------------------------------------------- error plumbing
static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail(AFR_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// Every entry point that enqueues work makes the device that owns the caller's buffers current for the duration of the
// call (and restores the previous one): kernels are launched on the caller's stream, which belongs to that device, so a
// process whose current device is another GPU (LOCAL_RANK != 0 without a set_device) still launches where the data lives.
static int device_of(const void* ptr) {
    hipPointerAttribute_t a;
    if (!ptr || hipPointerGetAttributes(&a, ptr) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return a.device;
}
struct DevGuard {
    int prev = -1; bool switched = false;
    explicit DevGuard(int dev) {
        if (dev < 0 || hipGetDevice(&prev) != hipSuccess || prev == dev) return;
        switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DevGuard() { if (switched) (void)hipSetDevice(prev); }
};

extern "C" int afr_version(void) { return AFR_VERSION; }
extern "C" const char* afr_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------------------ plan
struct Tensor {
    std::string name;
    int64_t off = 0, numel = 0;
    int ndim = 0;
    int64_t shape[4] = {0, 0, 0, 0};
};

struct ProfRec { int tag; hipEvent_t a, b; double flops, bytes; };
// The loss scratch of a plan (o_loss) or of an afr_op_*_grad caller, in floats: the loss kernel's own launch keeps its <= 1024
// partials at the front and its arrival counter behind them; a loss fused into another kernel (GEMM epilogue, small-net step)
// has a counter of its own and its partials, one per block of that launch, behind it.
constexpr int LOSS_WS_COUNTER = 1024, LOSS_WS_FUSED_COUNTER = 1032, LOSS_WS_FUSED_PARTIAL = 1040;
struct AdamArgs { float lr, b1, b2, eps, wd; int64_t t; };      // the optimizer arguments of afr_train_step
// The optimizer step ONE afr_train_step call is taking: made by train_step_impl and handed down to whatever applies part of it.
// The entry points that only run a backward hand none, so they can never see a step, or a deferred loss sum, that is not theirs.
struct StepCtx {
    AdamArgs h;
    int64_t done[AFR_MAX_HIDDEN + 1]; int ndone = 0;   // weights (flat offsets) a cooperative weight-gradient tail has stepped: one per Linear at most
    LossSum loss{};   // deferred loss: partials the forward's last GEMM stored without the ticket; the fused first-layer backward adds them
};
// The clip scratch of a plan (o_clip), in floats: grad_sumsq_kernel's scratch, the word its sum goes to, the segment table
constexpr int CLIP_WS_SUMSQ = AFR_SUMSQ_SCRATCH_FLOATS, CLIP_WS_TABLE = AFR_SUMSQ_SCRATCH_FLOATS + 8;
static_assert(CLIP_WS_TABLE * sizeof(float) % alignof(SumsqSeg) == 0, "the segment table is aligned");

struct afr_plan {
    afr_config cfg;                // cfg.dtype is the ACTIVATION dtype (AFR_F32 or AFR_BF16) every non-GEMM kernel runs in
    int gemm_dtype = AFR_F32;      // the dtype run_gemm launches its products in: cfg.dtype, or AFR_BF16X3 over f32 activations
    std::vector<Tensor> params;
    int64_t total = 0;
    int act_bytes = 4;
    // bound buffers
    float *P = nullptr, *G = nullptr, *M = nullptr, *V = nullptr;
    char* ws = nullptr;
    size_t ws_bytes = 0, ws_need = 0;
    int device = -1;               // the GPU that owns the bound buffers (afr_bind)
    // workspace offsets (bytes)
    size_t o_shadow = 0, o_err = 0, o_loss = 0, o_u = 0, o_z = 0, o_dz = 0, o_slab_e = 0, o_save = 0;
    std::vector<size_t> o_act;     // glyph: activations h0..h_nh
    size_t o_d[2] = {0, 0};        // glyph: ping-pong d buffers
    size_t o_table = 0;            // glyph: [Emb; Font] . W1^T, the first Linear folded through the tables
    size_t o_dw1 = 0;              // glyph: compact dW1 [N1][E] extracted from the widened weight-gradient slabs
    int k0 = 0;                    // glyph: columns of h0' = [h0 | one-hot] when the first layer is folded, else 0
    // glyph, one small hidden layer (BASELINE C1 / C2): the whole step as ONE fused kernel + the grouped reduce (glyph_fused.hip)
    bool fused1 = false;
    bool wT_valid = false;         // bf16: the transposed operand copies W1T / W2T match the current parameters
    size_t o_w1t = 0, o_w2t = 0, o_slab1 = 0;
    bool l1f = false; size_t o_l1f = 0;   // glyph, bf16: folded first layer's backward in one kernel (slabs [blocks][dW1|db1|dTab])
    // glyph, bf16 training steps: the first layer's output as a COMBINATION table (elementwise.hip glyph_combo_kernel): h1 / h0
    // are not materialised per glyph; the products that consume them gather table rows through cidx while staging
    bool combo_ok = false; size_t o_h1c = 0, o_h0c = 0, o_cidx = 0; int h1c_ld = 0;
    // glyph, bf16 training steps: hidden activations written by a GEMM epilogue also leave their ReLU mask as bits
    // (o_mbits[i] for the output of layer i, 0 = none); the next layer's input-gradient product reads those instead of the activation
    std::vector<size_t> o_mbits;
    // bf16 glyph nets: TWO weight shadows.  A fused optimizer step writes every tensor's new bf16 copy into the one that is
    // not being read (a layer's weight-gradient workgroups update the weights while the same launch's input-gradient
    // workgroups still read them), and the roles swap when the step is complete.
    size_t o_shadow2 = 0; int shadow_cur = 0;
    // bf16 glyph nets: the chained gradient launch (gemm.hip GemmGroup::chain) hands the output layer's input gradient to the hidden
    // layer's products inside ONE launch: a monotonic arrival counter per 256 rows of the batch (o_hand, 0 = none), the arrivals
    // enqueued so far, and the CUs of the bound device (a chain wants a CU per workgroup)
    // Behind those counters a second set of the same size: dX_lo's output handed to the first-layer role of the same launch
    // (GemmGroup::l1; l1_cnt_of), with its own arrivals enqueued so far
    size_t o_hand = 0; unsigned hand_arrived = 0; int n_cus = 0; unsigned l1_arrived = 0;
    // pixel-token transformer (AFR_KIND_PIXEL): per-block parameter offsets and the forward's workspace
    struct PixBlock { int64_t ln1g, ln1b, win, bin, wo, bo, ln2g, ln2b, w1, b1, w2, b2; };
    std::vector<PixBlock> pix;
    int64_t px_pos = 0, px_emb = 0, px_font = -1, px_lnfg = 0, px_lnfb = 0, px_wout = 0, px_bout = 0;
    struct PixSave { size_t hin, h1, n1, q, o, n2, kv, f, ln1p, ln2p, fbits; };      // per block: what its backward needs + its LayerNorm partial slabs
    std::vector<PixSave> pxs;
    size_t o_ctx = 0, o_a = 0, o_hf = 0, o_dh = 0, o_dht = 0, o_df = 0, o_dn = 0, o_dq = 0, o_dkvp = 0, o_dkv = 0, o_dkvt = 0, o_dctxt = 0,
           o_dctx = 0, o_headp = 0;
    // glyph layer table
    struct Layer { int N, K; int64_t w_off, b_off; int sk = 1; size_t o_slab_w = 0, o_slab_b = 0;
                   size_t o_cnt = 0; int n_cnt = 0; unsigned coop_arrived = 0; };   // cooperative split-K: per-tile arrival counters, arrivals enqueued so far
    std::vector<Layer> layers;
    std::vector<Layer> pxl;          // the 5 Linears of every block as weight-gradient descriptors: q, kv, out-proj, fc1, fc2
    int64_t emb_off = 0, font_off = 0;
    // sheet offsets
    int64_t s_pos = 0, s_emb = 0, s_win = 0, s_bin = 0, s_wo = 0, s_bo = 0, s_g = 0, s_b = 0, s_w1 = 0, s_b1 = 0, s_wout = 0, s_bout = 0;
    // What the last forward left for the loss, evaluation and backward entry points.  A forward (forward_impl's two exits, the
    // one-launch small-net step) sets ALL of it through forward_done; the calls after it only move have_du / have_u / next_stage.
    struct Last {
        const int64_t *x = nullptr, *font = nullptr;
        int B = 0, L = 0, ldx = 0, training = 0, next_stage = 0;
        uint64_t step = 0;
        bool have_du = false;         // the u buffer holds d(loss)/du: a backward may start
        bool have_u = false;          // the u buffer holds the pre-activation of the last forward (afr_eval*): not yet overwritten by du
        bool combo_on = false, mbits_on = false;   // glyph: the first layer ran as a combination table / the ReLU masks were left as bits
        enum Holds { NOTHING, U, DU };      // what the u buffer holds when the forward returns
        void forward_done(const int64_t* x_, const int64_t* font_, int B_, int L_, int ldx_, int training_, uint64_t step_, Holds h,
                          bool combo = false, bool mbits = false) {
            x = x_; font = font_; B = B_; L = L_; ldx = ldx_; training = training_; step = step_;
            have_du = h == DU; have_u = h == U; next_stage = 0; combo_on = combo; mbits_on = mbits;
        }
    } last;
    // the bound data set (afr_bind_dataset; caller-owned device buffers) and the workspace staging of the afr_*_rows calls: the
    // narrowed row indices the loss kernels' row maps read, and the batch's codes / font ids for the id consumers
    const int64_t* ds_x = nullptr; const int64_t* ds_font = nullptr; const void* ds_target = nullptr;
    int ds_tdtype = 0, ds_L = 0; int64_t ds_rows = 0;
    size_t o_ridx = 0, o_sx = 0, o_sfont = 0;
    // clipping by global gradient norm (afr_set_grad_clip): 0 = off; o_clip = [block partials + arrival counter | sumsq word |
    // the (offset, numel) table of the parameter tensors], uploaded / zeroed by afr_bind
    float clip_norm = 0.f; float* clip_stats = nullptr;
    int opt_kind = OPT_ADAMW;               // afr_set_optimizer: the update every optimizer step of the plan applies
    // optimizer groups (afr_set_param_groups): adjacent tensors with equal multipliers merged into ranges of the flat buffer, in
    // offset order, the last one ending at `total`; empty = off (one lr, one weight decay for every tensor)
    std::vector<afr_opt_range> groups;
    std::vector<SumsqSeg> clip_segs;        // host copy of that table
    size_t o_clip = 0;
    // per-tensor statistics (afr_tensor_stats): the partial records of launch 1, one per chunk of every tensor; tstats_ok is false
    // for a table the kernels do not take (more than 256 tensors, or one of 2^32 elements or more) and nothing is carved then
    size_t o_tstats = 0; bool tstats_ok = false;
    // weight EMA (afr_set_ema): E = the caller's buffer in the parameter layout (NULL = off), updated by every ema_every-th optimizer
    // step of the plan (ema_count of them since afr_set_ema).  ema_on (afr_use_ema): P and E have changed places, the forward
    // entry points read the EMA weights and every call that trains or steps is refused.
    float* E = nullptr; float ema_decay = 0.f; int ema_every = 1; int64_t ema_count = 0; bool ema_on = false;
    // profiling
    int prof_mode = 0;      // 0 off, 1 every launch, 2 only prof_only, 3 every 4th launch of prof_only
    unsigned prof_seen = 0; // launches of prof_only met in mode 3
    std::string prof_only_sym;   // mode 2: the kernel symbol to keep timing
    double prof_overhead_ms = -1.0;   // event-bracket overhead, measured on first use (prof_calibrate)
    std::vector<ProfRec> prof;
    std::vector<std::string> prof_tags;
    std::vector<hipEvent_t> ev_pool;
};

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// the folded first layer's backward is the ONE fused kernel (gemm.hip glyph_l1_bwd_fused_kernel), not GEMM + extraction
static inline bool l1_bwd_fused(const afr_plan* p) { return p->l1f && !(p->cfg.reserved & AFR_CFG_L1_BWD_UNFUSED); }

static void add_param(afr_plan* p, const char* name, std::initializer_list<int64_t> shape) {
    Tensor t;
    t.name = name;
    t.ndim = (int)shape.size();
    int64_t n = 1;
    int i = 0;
    for (int64_t s : shape) { t.shape[i++] = s; n *= s; }
    t.numel = n;
    t.off = p->total;
    p->total += (n + 63) / 64 * 64;
    p->params.push_back(t);
}
static int64_t off_of(const afr_plan* p, const char* name) {
    for (const Tensor& t : p->params)
        if (t.name == name) return t.off;
    return -1;
}

static_assert(AFR_RT_MAXSEG >= 2 * AFR_MAX_HIDDEN + 2 * AFR_L1F_MAX_SPLIT + 4, "a backward pass of the deepest glyph net must fit one grouped reduce");
static int choose_splitk(int M, int N, int K) {
    // a small weight gradient reduced over very many rows (the pixel transformer's: 131072 token rows into 2048 x 512): as many
    // K-slices as make the 256x256 tiles fill the chip exactly once -- the launcher then takes the 256x256 body for it
    // (gemm.hip bf16_use_body256; measured 323 -> 292 us and 287 -> 246 us against the best split of the 256x128 ring)
    const int t256 = ((M + 255) / 256) * ((N + 255) / 256);
    if (K >= 32768 && t256 >= 8 && t256 <= 64 && 256 % t256 == 0 && K / (256 / t256) >= 1024) return 256 / t256;
    const int tiles = ((M + 127) / 128) * ((N + 127) / 128);
    int s = (512 + tiles - 1) / tiles;                 // about 512 blocks of 128x128 tiles
    const int maxs = K / 256 > 0 ? K / 256 : 1;
    if (s > maxs) s = maxs;
    if (s < 1) s = 1;
    if (s > 64) s = 64;
    return s;
}

extern "C" int afr_plan_create(const afr_config* c, afr_plan** out) {
    if (!c || !out) return fail(AFR_EINVAL, "null argument");
    if (c->dtype != AFR_F32 && c->dtype != AFR_BF16 && c->dtype != AFR_BF16X3)
        return fail(AFR_EINVAL, "dtype must be AFR_F32, AFR_BF16 or AFR_BF16X3");
    if (c->loss != AFR_LOSS_MSE && c->loss != AFR_LOSS_BCE)
        return fail(AFR_EINVAL, "afr_config.loss must be AFR_LOSS_MSE (0) or AFR_LOSS_BCE (1), got %d", c->loss);
    // AFR_BF16X3 is the f32 plan (activations, layout, workspace, every non-GEMM kernel) whose products run bf16x3
    afr_config cf = *c;
    const int gemm_dtype = cf.dtype;
    if (cf.dtype == AFR_BF16X3) cf.dtype = AFR_F32;
    c = &cf;
    if (c->max_batch <= 0) return fail(AFR_EINVAL, "max_batch must be positive");
    if (c->vocab <= 0 || c->embed_dim <= 0 || c->out_h <= 0 || c->out_w <= 0) return fail(AFR_EINVAL, "bad shape");
    const int Pix = c->out_h * c->out_w;
    if (Pix % 8) return fail(AFR_EUNSUPPORTED, "out_h*out_w must be a multiple of 8 (got %d)", Pix);
    afr_plan* p = new afr_plan();
    p->cfg = *c;
    p->gemm_dtype = gemm_dtype;
    p->act_bytes = c->dtype == AFR_BF16 ? 2 : 4;
    const int E = c->embed_dim;
    const size_t B = (size_t)c->max_batch;
    const size_t ab = (size_t)p->act_bytes;
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };

    if (c->kind == AFR_KIND_SHEET) {
        if (E != 32 || c->heads != 4 || c->fc_dim != 64)
            { delete p; return fail(AFR_EUNSUPPORTED, "sheet front end is built for embed_dim 32, 4 heads, fc_dim 64 (model.py:79,81,148)"); }
        if (c->max_length <= 0 || c->max_length > 120) { delete p; return fail(AFR_EUNSUPPORTED, "max_length must be in 1..120 (one string's state must fit 160 KiB of LDS)"); }
        const int L = c->max_length, F = c->fc_dim;
        add_param(p, "positional_encoding", {L, E});
        add_param(p, "embedding.weight", {c->vocab, E});
        add_param(p, "attention.in_proj_weight", {3 * E, E});
        add_param(p, "attention.in_proj_bias", {3 * E});
        add_param(p, "attention.out_proj.weight", {E, E});
        add_param(p, "attention.out_proj.bias", {E});
        add_param(p, "layer_norm.weight", {E});
        add_param(p, "layer_norm.bias", {E});
        add_param(p, "fc1.weight", {F, E});
        add_param(p, "fc1.bias", {F});
        add_param(p, "fc_output.weight", {Pix, (int64_t)L * F});
        add_param(p, "fc_output.bias", {Pix});
        p->s_pos = off_of(p, "positional_encoding"); p->s_emb = off_of(p, "embedding.weight");
        p->s_win = off_of(p, "attention.in_proj_weight"); p->s_bin = off_of(p, "attention.in_proj_bias");
        p->s_wo = off_of(p, "attention.out_proj.weight"); p->s_bo = off_of(p, "attention.out_proj.bias");
        p->s_g = off_of(p, "layer_norm.weight"); p->s_b = off_of(p, "layer_norm.bias");
        p->s_w1 = off_of(p, "fc1.weight"); p->s_b1 = off_of(p, "fc1.bias");
        p->s_wout = off_of(p, "fc_output.weight"); p->s_bout = off_of(p, "fc_output.bias");
        const size_t Kz = (size_t)L * F;
        if (c->dtype == AFR_BF16) p->o_shadow = carve((size_t)p->total * 2);
        p->o_err = carve(256);
        p->o_loss = carve(((size_t)((B + 127) / 128) * ((Pix + 127) / 128) + LOSS_WS_FUSED_PARTIAL) * sizeof(float));
        p->o_z = carve(B * Kz * ab);
        p->o_u = carve(B * Pix * ab);
        p->o_dz = carve(B * Kz * ab);
        afr_plan::Layer ly; ly.N = Pix; ly.K = (int)Kz; ly.w_off = p->s_wout; ly.b_off = p->s_bout;
        ly.sk = choose_splitk(Pix, (int)Kz, (int)B);
        if (ly.sk > 1) { ly.o_slab_w = carve((size_t)ly.sk * Pix * Kz * sizeof(float)); ly.o_slab_b = carve((size_t)ly.sk * Pix * sizeof(float)); }
        p->layers.push_back(ly);
        p->o_slab_e = carve((size_t)afr_sheet_blocks((int)B) * (size_t)p->s_wout * sizeof(float));
        p->o_save = carve(B * (size_t)L * AFR_SHEET_SAVE_PER_POS * sizeof(float));
    } else if (c->kind == AFR_KIND_GLYPH) {
        if (c->n_hidden < 0 || c->n_hidden > AFR_MAX_HIDDEN) { delete p; return fail(AFR_EINVAL, "n_hidden out of range"); }
        if (E % 8) { delete p; return fail(AFR_EUNSUPPORTED, "embed_dim must be a multiple of 8"); }
        for (int i = 0; i < c->n_hidden; ++i)
            if (c->hidden[i] <= 0 || c->hidden[i] % 8) { delete p; return fail(AFR_EUNSUPPORTED, "hidden widths must be positive multiples of 8"); }
        add_param(p, "embedding.weight", {c->vocab, E});
        if (c->n_fonts > 0) add_param(p, "font_embedding.weight", {c->n_fonts, E});
        int k = E;
        char nm[64];
        for (int i = 0; i < c->n_hidden; ++i) {
            snprintf(nm, sizeof nm, "fc%d.weight", i + 1);
            add_param(p, nm, {c->hidden[i], k});
            afr_plan::Layer ly; ly.N = c->hidden[i]; ly.K = k; ly.w_off = p->params.back().off;
            snprintf(nm, sizeof nm, "fc%d.bias", i + 1);
            add_param(p, nm, {c->hidden[i]});
            ly.b_off = p->params.back().off;
            p->layers.push_back(ly);
            k = c->hidden[i];
        }
        add_param(p, "fc_output.weight", {Pix, k});
        afr_plan::Layer ly; ly.N = Pix; ly.K = k; ly.w_off = p->params.back().off;
        add_param(p, "fc_output.bias", {Pix});
        ly.b_off = p->params.back().off;
        p->layers.push_back(ly);
        p->emb_off = off_of(p, "embedding.weight");
        p->font_off = c->n_fonts > 0 ? off_of(p, "font_embedding.weight") : -1;
        if (c->dtype == AFR_BF16) { p->o_shadow = carve((size_t)p->total * 2); p->o_shadow2 = carve((size_t)p->total * 2); }
        p->o_err = carve(256);
        p->o_loss = carve(((size_t)((B + 127) / 128) * ((Pix + 127) / 128) + LOSS_WS_FUSED_PARTIAL) * sizeof(float));
        size_t maxw = (size_t)E, maxn = 0;
        p->k0 = c->n_hidden > 0 ? afr_glyph_k0(E, c->vocab, c->n_fonts) : 0;
        if (p->k0 > 512 || E > 128) p->k0 = 0;     // beyond what the folded-layer kernels stage per block: plain embedding + GEMM path
        p->o_act.push_back(carve(B * (size_t)(p->k0 ? p->k0 : E) * ab));
        for (int i = 0; i < c->n_hidden; ++i) {
            p->o_act.push_back(carve(B * (size_t)c->hidden[i] * ab));
            if ((size_t)c->hidden[i] > maxw) maxw = (size_t)c->hidden[i];
        }
        p->o_mbits.assign(c->n_hidden + 1, 0);
        if (c->dtype == AFR_BF16 && !(c->reserved & AFR_CFG_RELU_MASK_FROM_ACT))
            for (int i = 1; i < c->n_hidden; ++i)          // layer 0's output comes from the table / gather kernels, not a GEMM
                if (c->hidden[i] % 8 == 0) p->o_mbits[i] = carve(B * (size_t)(c->hidden[i] / 8));
        p->o_u = carve(B * Pix * ab);
        p->o_d[0] = carve(B * maxw * ab);
        p->o_d[1] = carve(B * maxw * ab);
        bool first = true;
        for (auto& l : p->layers) {
            // the folded first layer's weight-gradient GEMM is K0 wide and always lands in slabs (even a single one)
            const int kw = (first && p->k0) ? p->k0 : l.K;
            l.sk = choose_splitk(l.N, kw, (int)B);
            // (slab space in whole 256x256 tiles: the cooperative split-K parks register images of full tiles there)
            const size_t wt = (size_t)((l.N + 255) / 256) * ((kw + 255) / 256);
            if (l.sk > 1 || (first && p->k0)) { l.o_slab_w = carve((size_t)l.sk * wt * 65536 * sizeof(float)); l.o_slab_b = carve((size_t)l.sk * l.N * sizeof(float)); }
            l.n_cnt = (int)wt; l.o_cnt = carve(wt * sizeof(unsigned));
            if ((size_t)l.N > maxn) maxn = (size_t)l.N;
            first = false;
        }
        size_t eb = (size_t)afr_embed_bwd_blocks((int)B);
        if (p->k0) {
            const size_t lb = (size_t)afr_glyph_l1_bwd_blocks(c->hidden[0]);
            if (lb > eb) eb = lb;
            p->o_table = carve((size_t)(c->vocab + c->n_fonts) * c->hidden[0] * sizeof(float));
            p->o_dw1 = carve((size_t)c->hidden[0] * E * sizeof(float));
            if (afr_glyph_l1_bwd_fused_eligible(c->dtype, E, c->hidden[0], c->vocab, c->n_fonts)) {
                p->l1f = true;
                // worst case over batch sizes <= max_batch: every 64-glyph block with the full-width slab, or 256 blocks of the narrowest
                p->o_l1f = carve(((size_t)((B + 63) / 64) + 256) * (size_t)((size_t)c->hidden[0] * E + c->hidden[0] + (size_t)(c->vocab + c->n_fonts) * E) * sizeof(float));
                p->o_w1t = carve((size_t)c->hidden[0] * E * 2);
            }
        }
        // the plain embedding path's backward (glyph_embed_bwd_kernel) keeps the whole table's accumulator in one block's LDS
        if (!p->k0 && afr_glyph_embed_bwd_lds_bytes(E, c->vocab, c->n_fonts) > 160 * 1024) {
            delete p;
            return fail(AFR_EUNSUPPORTED, "glyph net without a folded first layer: the embedding backward needs %zu bytes of LDS for (vocab + n_fonts) x embed_dim = %d x %d, above 160 KiB",
                        afr_glyph_embed_bwd_lds_bytes(E, c->vocab, c->n_fonts), c->vocab + c->n_fonts, E);
        }
        p->o_slab_e = carve(eb * (size_t)(c->vocab + c->n_fonts) * E * sizeof(float));
        {
            const size_t ncombo = (size_t)c->vocab * (c->n_fonts > 0 ? c->n_fonts : 1);
            if (c->dtype == AFR_BF16 && l1_bwd_fused(p) && c->n_hidden >= 2 && ncombo <= 1024 && !(c->reserved & AFR_CFG_NO_COMBO_TABLE)) {
                p->combo_ok = true;
                p->h1c_ld = c->hidden[0];
                p->o_h1c = carve(ncombo * p->h1c_ld * 2); p->o_h0c = carve(ncombo * E * 2); p->o_cidx = carve(B * sizeof(int));
            }
        }
        if (c->n_hidden == 1 && afr_glyph1_eligible(E, c->hidden[0], Pix, c->vocab, c->n_fonts) &&
            afr_glyph1_lds_bytes(c->dtype, E, c->hidden[0], Pix, c->vocab + c->n_fonts) <= 160 * 1024) {
            p->fused1 = true;
            const size_t nblk = (size_t)afr_glyph1_max_blocks(c->dtype, (int)B, Pix);      // row blocks x column split
            p->o_slab1 = carve(nblk * (size_t)p->total * sizeof(float));
            p->o_loss = carve((LOSS_WS_FUSED_PARTIAL + nblk + 64) * sizeof(float));           // room for one loss partial per block
            if (c->dtype == AFR_BF16) {
                if (!p->l1f) p->o_w1t = carve((size_t)c->hidden[0] * E * 2);
                p->o_w2t = carve((size_t)Pix * c->hidden[0] * 2);
            }
        }
    } else if (c->kind == AFR_KIND_PIXEL) {
        const int d = E, ff = c->fc_dim, T = Pix, nf = c->n_fonts > 0 ? c->n_fonts : 0, C = nf > 0 ? 2 : 1;
        if (d > 512 || d % 64 || c->heads * 64 != d || ff <= 0 || ff % 8 || c->n_hidden < 1 || c->n_hidden > AFR_MAX_HIDDEN)
            { delete p; return fail(AFR_EUNSUPPORTED, "pixel transformer: d_model = 64 * heads <= 512, ff a multiple of 8, 1..%d blocks", AFR_MAX_HIDDEN); }
        add_param(p, "positional_encoding", {T, d});
        add_param(p, "embedding.weight", {c->vocab, d});
        if (nf > 0) add_param(p, "font_embedding.weight", {nf, d});
        char nm[64];
        for (int l = 0; l < c->n_hidden; ++l) {
            afr_plan::PixBlock b;
            auto addp = [&](const char* suffix, std::initializer_list<int64_t> shape) { snprintf(nm, sizeof nm, "layers.%d.%s", l, suffix); add_param(p, nm, shape); return p->params.back().off; };
            b.ln1g = addp("ln1.weight", {d}); b.ln1b = addp("ln1.bias", {d});
            b.win = addp("attn.in_proj_weight", {3 * d, d}); b.bin = addp("attn.in_proj_bias", {3 * d});
            b.wo = addp("attn.out_proj.weight", {d, d}); b.bo = addp("attn.out_proj.bias", {d});
            b.ln2g = addp("ln2.weight", {d}); b.ln2b = addp("ln2.bias", {d});
            b.w1 = addp("fc1.weight", {ff, d}); b.b1 = addp("fc1.bias", {ff});
            b.w2 = addp("fc2.weight", {d, ff}); b.b2 = addp("fc2.bias", {d});
            p->pix.push_back(b);
        }
        add_param(p, "ln_f.weight", {d}); add_param(p, "ln_f.bias", {d});
        add_param(p, "fc_output.weight", {1, d}); add_param(p, "fc_output.bias", {1});
        p->px_pos = off_of(p, "positional_encoding"); p->px_emb = off_of(p, "embedding.weight");
        p->px_font = nf > 0 ? off_of(p, "font_embedding.weight") : -1;
        p->px_lnfg = off_of(p, "ln_f.weight"); p->px_lnfb = off_of(p, "ln_f.bias");
        p->px_wout = off_of(p, "fc_output.weight"); p->px_bout = off_of(p, "fc_output.bias");
        const size_t rows = B * (size_t)T;
        if (c->dtype == AFR_BF16 && (rows * (size_t)(ff > d ? ff : d) * 2 >= (1ull << 31)))
            { delete p; return fail(AFR_EUNSUPPORTED, "max_batch %d x %d tokens: an activation operand would reach 2 GiB in bf16", c->max_batch, T); }
        if (c->dtype == AFR_BF16) p->o_shadow = carve((size_t)p->total * 2);
        p->o_err = carve(256);
        p->o_loss = carve((LOSS_WS_FUSED_PARTIAL + 1040) * sizeof(float));
        p->o_ctx = carve(B * C * d * ab);
        const size_t nbp = (size_t)afr_pixel_bwd_blocks((long long)rows);
        for (int l = 0; l < c->n_hidden; ++l) {
            afr_plan::PixSave sv;
            sv.hin = carve(rows * d * sizeof(float)); sv.h1 = carve(rows * d * sizeof(float));
            sv.n1 = carve(rows * d * ab); sv.q = carve(rows * d * ab); sv.o = carve(rows * d * ab); sv.n2 = carve(rows * d * ab);
            sv.kv = carve(B * C * 2 * d * ab); sv.f = carve(rows * ff * ab);
            sv.fbits = c->dtype == AFR_BF16 ? carve(rows * (size_t)(ff / 8)) : 0;      // ReLU gate of F, one byte per 8 columns (bf16 mode)
            sv.ln1p = carve(nbp * 2 * d * sizeof(float)); sv.ln2p = carve(nbp * 2 * d * sizeof(float));
            p->pxs.push_back(sv);
            const afr_plan::PixBlock& b = p->pix[l];
            const struct { int N, K; int64_t w, bo; long long red; } lin[5] = {
                {d, d, b.win, b.bin, (long long)rows}, {2 * d, d, b.win + (int64_t)d * d, b.bin + d, (long long)(B * C)}, {d, d, b.wo, b.bo, (long long)rows},
                {ff, d, b.w1, b.b1, (long long)rows}, {d, ff, b.w2, b.b2, (long long)rows}};
            for (const auto& q_ : lin) {
                afr_plan::Layer ly; ly.N = q_.N; ly.K = q_.K; ly.w_off = q_.w; ly.b_off = q_.bo;
                ly.sk = choose_splitk(q_.N, q_.K, (int)(q_.red > 0x7fffffff ? 0x7fffffff : q_.red));
                if (ly.sk > 1) { ly.o_slab_w = carve((size_t)ly.sk * q_.N * q_.K * sizeof(float)); ly.o_slab_b = carve((size_t)ly.sk * q_.N * sizeof(float)); }
                p->pxl.push_back(ly);
            }
        }
        p->o_a = carve(rows * d * ab); p->o_hf = carve(rows * d * sizeof(float));
        p->o_u = carve(rows * sizeof(float));
        p->o_dh = carve(rows * d * sizeof(float)); p->o_dht = c->dtype == AFR_BF16 ? carve(rows * d * ab) : 0;
        p->o_df = carve(rows * ff * ab); p->o_dn = carve(rows * d * ab); p->o_dq = carve(rows * d * ab);
        const size_t chunks = ((size_t)T + afr_pixel_attn_chunk(T) - 1) / afr_pixel_attn_chunk(T);
        p->o_dkvp = carve(B * chunks * 4 * d * sizeof(float)); p->o_dkv = carve(B * 4 * d * sizeof(float)); p->o_dkvt = carve(B * C * 2 * d * ab);
        p->o_dctxt = carve(B * C * d * ab); p->o_dctx = carve(B * C * d * sizeof(float));
        p->o_headp = carve(nbp * 4 * d * sizeof(float));
    } else {
        delete p;
        return fail(AFR_EINVAL, "unknown model kind %d", c->kind);
    }
    if (c->dtype == AFR_BF16) {
        // every bf16 GEMM operand (activations [max_batch][width], weight shadows) is addressed with 32-bit byte offsets
        long long widest = Pix;
        for (const auto& l : p->layers) { if (l.N > widest) widest = l.N; if (l.K > widest) widest = l.K; }
        if ((long long)c->max_batch * widest * 2 >= (1ll << 31)) {
            const long long lim = ((1ll << 31) - 1) / (widest * 2);
            delete p;
            return fail(AFR_EUNSUPPORTED, "max_batch %d too large for bf16 mode: an activation operand would reach 2 GiB (limit %lld rows of %lld)", c->max_batch, lim, widest);
        }
        for (const auto& l : p->layers)
            if ((long long)l.N * l.K * 2 >= (1ll << 31)) { delete p; return fail(AFR_EUNSUPPORTED, "a %d x %d weight is 2 GiB or more in bf16", l.N, l.K); }
    }
    // staging of the afr_*_rows calls: row indices int [max_batch], codes int64 [max_batch][max_length or 1], font ids int64 [max_batch]
    p->o_ridx = carve(B * sizeof(int));
    p->o_sx = carve(B * (size_t)(c->kind == AFR_KIND_SHEET ? c->max_length : 1) * sizeof(int64_t));
    p->o_sfont = carve(B * sizeof(int64_t));
    for (const Tensor& t : p->params) p->clip_segs.push_back(SumsqSeg{(long long)t.off, (long long)t.numel});
    p->o_clip = carve(CLIP_WS_TABLE * sizeof(float) + p->clip_segs.size() * sizeof(SumsqSeg));
    {   // the statistics' partials, behind everything else: no existing offset moves
        long long chunks = 0;
        p->tstats_ok = p->clip_segs.size() <= (size_t)AFR_TSTATS_MAX_SEGS;
        for (const SumsqSeg& sg : p->clip_segs) { chunks += afr_tstats_seg_blocks(sg.numel); if (sg.numel > 0xffffffffll) p->tstats_ok = false; }
        if (p->tstats_ok) p->o_tstats = carve((size_t)chunks * sizeof(afr_tensor_stat));
    }
    if (c->kind == AFR_KIND_GLYPH && c->dtype == AFR_BF16 && p->layers.size() >= 3)      // (behind everything else as well)
        p->o_hand = carve(2 * (((size_t)c->max_batch + 255) / 256) * sizeof(unsigned));
    p->ws_need = off;
    *out = p;
    return AFR_OK;
}

extern "C" int afr_plan_destroy(afr_plan* p) {
    if (!p) return AFR_OK;
    for (hipEvent_t e : p->ev_pool) (void)hipEventDestroy(e);
    for (auto& r : p->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    delete p;
    return AFR_OK;
}

extern "C" int64_t afr_param_elems(const afr_plan* p) { return p ? p->total : 0; }
extern "C" int afr_param_count(const afr_plan* p) { return p ? (int)p->params.size() : 0; }
extern "C" int afr_param_info(const afr_plan* p, int i, char* name, int cap, int64_t* offset, int64_t* numel,
                              int32_t* ndim, int64_t shape[4]) {
    if (!p || i < 0 || i >= (int)p->params.size()) return fail(AFR_EINVAL, "parameter index out of range");
    const Tensor& t = p->params[i];
    if (name && cap > 0) { strncpy(name, t.name.c_str(), cap - 1); name[cap - 1] = 0; }
    if (offset) *offset = t.off;
    if (numel) *numel = t.numel;
    if (ndim) *ndim = t.ndim;
    if (shape) for (int k = 0; k < 4; ++k) shape[k] = t.shape[k];
    return AFR_OK;
}
extern "C" size_t afr_workspace_bytes(const afr_plan* p) { return p ? p->ws_need : 0; }

extern "C" int afr_bind(afr_plan* p, float* params, float* grads, float* m, float* v, void* ws, size_t ws_bytes) {
    if (!p || !params || !ws) return fail(AFR_EINVAL, "params and workspace are required");
    if (p->ema_on) return fail(AFR_ESTATE, "afr_bind while the plan reads its EMA weights: afr_use_ema(plan, 0) first");
    if (ws_bytes < p->ws_need) return fail(AFR_EINVAL, "workspace too small: %zu < %zu", ws_bytes, p->ws_need);
    if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ws) & 255)
        return fail(AFR_EINVAL, "buffers must be 256-byte aligned");
    const int dev = device_of(params);
    for (const void* q : {(const void*)grads, (const void*)m, (const void*)v, (const void*)ws}) {
        const int d = device_of(q);
        if (q && d >= 0 && dev >= 0 && d != dev) return fail(AFR_EINVAL, "buffers live on different devices (%d and %d)", dev, d);
    }
    p->device = dev;
    p->P = params; p->G = grads; p->M = m; p->V = v;
    p->ws = (char*)ws; p->ws_bytes = ws_bytes;
    p->last.have_du = false; p->last.have_u = false;
    p->wT_valid = false;
    p->shadow_cur = 0;
    for (auto& l : p->layers) {                          // cooperative split-K: arrival counters and their host count start at zero
        l.coop_arrived = 0;
        if (l.n_cnt) { DevGuard dg(dev); HIPCHK(hipMemset(p->ws + l.o_cnt, 0, (size_t)l.n_cnt * sizeof(unsigned))); }
    }
    p->hand_arrived = 0; p->n_cus = 0; p->l1_arrived = 0;
    if (p->o_hand) {                                     // the chain's hand-off counters likewise; the device's CUs decide whether it chains
        DevGuard dg(dev);
        HIPCHK(hipMemset(p->ws + p->o_hand, 0, 2 * (((size_t)p->cfg.max_batch + 255) / 256) * sizeof(unsigned)));
        int d = 0;
        if (hipGetDevice(&d) == hipSuccess) (void)hipDeviceGetAttribute(&p->n_cus, hipDeviceAttributeMultiprocessorCount, d);
    }
    {   // the norm kernel's scratch starts at zero (it leaves it so) and its table of tensor elements is the parameter table
        DevGuard dg(dev);
        HIPCHK(hipMemset(p->ws + p->o_clip, 0, CLIP_WS_TABLE * sizeof(float)));
        HIPCHK(hipMemcpy(p->ws + p->o_clip + CLIP_WS_TABLE * sizeof(float), p->clip_segs.data(), p->clip_segs.size() * sizeof(SumsqSeg),
                         hipMemcpyHostToDevice));
    }
    return AFR_OK;
}

// ---------------------------------------------------------------------------------- profiling
static hipEvent_t ev_get(afr_plan* p) {
    if (!p->ev_pool.empty()) { hipEvent_t e = p->ev_pool.back(); p->ev_pool.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}
static int tag_id(afr_plan* p, const char* tag) {
    for (size_t i = 0; i < p->prof_tags.size(); ++i)
        if (p->prof_tags[i] == tag) return (int)i;
    p->prof_tags.push_back(tag);
    return (int)p->prof_tags.size() - 1;
}
// What an (event, launch, event) bracket adds to the kernel's own duration.  Two events recorded back to back with
// nothing in between are ~4.5 us apart on this part (two command-processor packets); a bracketed launch pays for ONE of
// them beyond the kernel (the closing record), i.e. half that interval: measured against rocprofv3's kernel durations the
// raw brackets read 2.6 us high, the full interval subtracted 1.9 us low, half of it within 0.5 us.  Measured once per
// plan, the first time profiling is on, and subtracted from every bracket.
static void prof_calibrate(afr_plan* p, hipStream_t s) {
    p->prof_overhead_ms = 0.0;
    float best = 1e9f;
    for (int i = 0; i < 16; ++i) {
        hipEvent_t a = ev_get(p), b = ev_get(p);
        if (hipEventRecord(a, s) != hipSuccess || hipEventRecord(b, s) != hipSuccess || hipEventSynchronize(b) != hipSuccess) return;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, a, b) == hipSuccess && ms < best) best = ms;
        p->ev_pool.push_back(a); p->ev_pool.push_back(b);
    }
    if (best < 1e8f) p->prof_overhead_ms = 0.5 * best;
}
// "gemm_bf16<1,1,4>[1024x1024x8192]" -> "gemm_bf16<1,1,4>": the symbol rocprofv3 reports; launches of one symbol with
// different shapes are recorded apart (per-shape table) and summed per symbol when the dominant KERNEL is picked
static std::string symbol_of(const std::string& tag) { return tag.substr(0, tag.find('[')); }
struct ProfScope {
    afr_plan* p; hipStream_t s; ProfRec r; bool on;
    ProfScope(afr_plan* p_, hipStream_t s_, const char* tag, double flops, double bytes) : p(p_), s(s_), on(p_->prof_mode != 0) {
        if (!on) return;
        if (p->prof_overhead_ms < 0.0) prof_calibrate(p, s);
        r.tag = tag_id(p, tag);
        if (p->prof_mode >= 2 && symbol_of(p->prof_tags[r.tag]) != p->prof_only_sym) { on = false; return; }
        if (p->prof_mode == 3 && (p->prof_seen++ & 3u)) { on = false; return; }     // a sample: every 4th launch
        r.flops = flops; r.bytes = bytes; r.a = ev_get(p); r.b = ev_get(p);
        (void)hipEventRecord(r.a, s);
    }
    ~ProfScope() { if (on) { (void)hipEventRecord(r.b, s); p->prof.push_back(r); } }
};
static int prof_totals(afr_plan* p, std::vector<double>& tot, std::vector<double>& fl, std::vector<double>& by,
                       std::vector<int64_t>& cnt) {
    const size_t n = p->prof_tags.size();
    tot.assign(n, 0.0); fl.assign(n, 0.0); by.assign(n, 0.0); cnt.assign(n, 0);
    for (auto& r : p->prof) {
        HIPCHK(hipEventSynchronize(r.b));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, r.a, r.b));
        ms = ms > (float)p->prof_overhead_ms ? ms - (float)p->prof_overhead_ms : 0.f;
        tot[r.tag] += ms; fl[r.tag] += r.flops; by[r.tag] += r.bytes; cnt[r.tag]++;
    }
    return AFR_OK;
}
// per-symbol sums of a per-tag table
struct SymAgg { std::string sym; double tot = 0, fl = 0, by = 0; int64_t cnt = 0; };
static std::vector<SymAgg> prof_by_symbol(afr_plan* p, const std::vector<double>& tot, const std::vector<double>& fl,
                                          const std::vector<double>& by, const std::vector<int64_t>& cnt) {
    std::vector<SymAgg> out;
    for (size_t i = 0; i < tot.size(); ++i) {
        if (!cnt[i]) continue;
        const std::string sy = symbol_of(p->prof_tags[i]);
        size_t k = 0;
        while (k < out.size() && out[k].sym != sy) ++k;
        if (k == out.size()) { out.emplace_back(); out[k].sym = sy; }
        out[k].tot += tot[i]; out[k].fl += fl[i]; out[k].by += by[i]; out[k].cnt += cnt[i];
    }
    return out;
}
extern "C" int afr_profile_dominant(afr_plan* p, int mode) {
    if (!p) return fail(AFR_EINVAL, "null plan");
    if (mode == 2 || mode == 3) {     // keep timing only the kernel (symbol) that dominated the launches recorded so far
        if (p->prof.empty() && p->prof_only_sym.empty())
            return fail(AFR_ESTATE, "mode 2 needs a mode-1 recording to pick the dominant kernel from");
        if (!p->prof.empty() && p->prof_mode == 1) {
            std::vector<double> tot, fl, by; std::vector<int64_t> cnt;
            int rc = prof_totals(p, tot, fl, by, cnt);
            if (rc) return rc;
            const std::vector<SymAgg> ag = prof_by_symbol(p, tot, fl, by, cnt);
            size_t best = 0;
            for (size_t i = 1; i < ag.size(); ++i) if (ag[i].tot > ag[best].tot) best = i;
            p->prof_only_sym = ag[best].sym;
        }
    }
    for (auto& r : p->prof) { p->ev_pool.push_back(r.a); p->ev_pool.push_back(r.b); }
    p->prof.clear();
    p->prof_mode = mode;
    p->prof_seen = 0;
    return AFR_OK;
}
extern "C" int afr_profile_read(afr_plan* p, char* name, int cap, double* avg_ms, int64_t* launches, double* flops,
                                double* bytes) {
    if (!p) return fail(AFR_EINVAL, "null plan");
    if (p->prof.empty()) return fail(AFR_ESTATE, "no profiled launches recorded");
    std::vector<double> tot, fl, by; std::vector<int64_t> cnt;
    int rc = prof_totals(p, tot, fl, by, cnt);
    if (rc) return rc;
    const std::vector<SymAgg> ag = prof_by_symbol(p, tot, fl, by, cnt);
    size_t best = 0;
    for (size_t i = 1; i < ag.size(); ++i) if (ag[i].tot > ag[best].tot) best = i;
    if (name && cap > 0) { strncpy(name, ag[best].sym.c_str(), cap - 1); name[cap - 1] = 0; }
    if (avg_ms) *avg_ms = ag[best].tot / (double)ag[best].cnt;
    if (launches) *launches = ag[best].cnt;
    if (flops) *flops = ag[best].fl / (double)ag[best].cnt;
    if (bytes) *bytes = ag[best].by / (double)ag[best].cnt;
    return AFR_OK;
}

extern "C" int afr_profile_dump(afr_plan* p, char* buf, int cap) {
    if (!p || !buf || cap <= 0) return fail(AFR_EINVAL, "bad arguments");
    std::vector<double> tot, fl, by; std::vector<int64_t> cnt;
    int rc = prof_totals(p, tot, fl, by, cnt);
    if (rc) return rc;
    int n = 0;
    buf[0] = 0;
    for (size_t i = 0; i < tot.size() && n < cap - 1; ++i) {
        if (!cnt[i]) continue;
        n += snprintf(buf + n, cap - n, "%s\t%lld\t%.6f\t%.6f\t%.6g\t%.6g\n", p->prof_tags[i].c_str(), (long long)cnt[i], tot[i],
                      tot[i] / cnt[i], fl[i] / cnt[i], by[i] / cnt[i]);
    }
    return AFR_OK;
}

// ------------------------------------------------------------------------------------ helpers
static LossArgs loss_slots(LossArgs l, float* scratch, bool fused) {
    l.partial = scratch + (fused ? LOSS_WS_FUSED_PARTIAL : 0);
    l.counter = reinterpret_cast<unsigned*>(scratch + (fused ? LOSS_WS_FUSED_COUNTER : LOSS_WS_COUNTER));
    return l;
}
// what every loss site is handed (rowmap: targets of batch row b = row rowmap[b] of `target`, afr_*_rows; NULL = row b)
static LossArgs loss_args(float* scratch, bool fused, int kind, const void* target, int tdtype, const int* rowmap, int64_t mean_elems, float* loss_accum) {
    LossArgs l;
    l.target = target; l.rowmap = rowmap; l.tdtype = tdtype; l.inv_n = (float)(1.0 / (double)mean_elems); l.loss_accum = loss_accum; l.kind = kind;
    return loss_slots(l, scratch, fused);
}
static LossArgs loss_args(const afr_plan* p, bool fused, const void* target, int tdtype, const int* rowmap, int64_t mean_elems, float* loss_accum) {
    return loss_args((float*)(p->ws + p->o_loss), fused, p->cfg.loss, target, tdtype, rowmap, mean_elems, loss_accum);
}
// the scalars of an AdamW step (torch.optim.AdamW, bias corrections in double as torch takes them); OPT_LION: decay, b1, b2 and
// step = lr -- no bias correction, eps and t are not read.  Lion's decay is the rounded product subtracted from one, never a fused
// multiply-add: the elementwise kernel folds the same two roundings on the device.
static AdamHyper adam_hyper(const AdamArgs& h, int kind = OPT_ADAMW) {
    if (kind == OPT_LION) {
#pragma clang fp contract(off)
        const float lw = h.lr * h.wd;
        return AdamHyper{1.f - lw, h.b1, h.b2, 0.f, h.lr, 1.f};
    }
    const float bc1 = (float)(1.0 - std::pow((double)h.b1, (double)h.t));
    const float bc2 = (float)(1.0 - std::pow((double)h.b2, (double)h.t));
    return AdamHyper{1.f - h.lr * h.wd, h.b1, h.b2, h.eps, h.lr / bc1, (float)(1.0 / std::sqrt((double)bc2))};
}
// the step count every entry point that takes an optimizer step checks before its first launch (1 - beta^0 = 0 divides)
static int check_step_count(int64_t t) { return t < 1 ? fail(AFR_EINVAL, "t starts at 1") : AFR_OK; }
// ---- optimizer groups: the ONE place a tensor's (lr_i, wd_i) are formed; every site that steps takes them from here
static inline float mul_f32(float a, float b) {      // one rounded product, never contracted into what follows
#pragma clang fp contract(off)
    return a * b;
}
static inline AdamArgs group_args(const AdamArgs& h, const afr_opt_range& r) {
    AdamArgs a = h;
    a.lr = mul_f32(h.lr, r.lr_mult); a.wd = mul_f32(h.wd, r.wd_mult);
    return a;
}
static const afr_opt_range* range_at(const afr_plan* p, int64_t off) {      // the range that holds flat element `off` (groups on)
    for (const afr_opt_range& r : p->groups) if (off < r.end) return &r;
    return &p->groups.back();
}
// the optimizer arguments of the tensor at flat offset `off`: the step's own when the plan has no groups
static inline AdamArgs args_at(const afr_plan* p, const AdamArgs& h, int64_t off) {
    return p->groups.empty() ? h : group_args(h, *range_at(p, off));
}
static bool mult_ok(float v) { return v >= 0.f && !std::isinf(v); }      // (false for NaN)
// The kernel's table for the slice [first, first + n) from ranges in flat coordinates: the ranges that end at or before `first`
// and those that begin at or after the slice's end are left out; lr_i, wd_i and step_i are folded here, by adam_hyper.
static int build_range_tab(const afr_opt_range* r, int nr, int64_t first, int64_t n, const AdamArgs& h, int kind, OptRangeTab& tab) {
    if (!r || nr < 1) return fail(AFR_EINVAL, "optimizer groups: no ranges");
    if (first < 0 || n < 0 || ((first | n) & 3)) return fail(AFR_EINVAL, "optimizer groups: first = %lld and n = %lld must be non-negative multiples of 4", (long long)first, (long long)n);
    int64_t prev = 0;
    for (int k = 0; k < nr; ++k) {
        if (r[k].end <= prev || (r[k].end & 3)) return fail(AFR_EINVAL, "optimizer groups: range ends must be multiples of 4 and strictly increasing (range %d ends at %lld)", k, (long long)r[k].end);
        if (!mult_ok(r[k].lr_mult) || !mult_ok(r[k].wd_mult)) return fail(AFR_EINVAL, "optimizer groups: the multipliers of range %d must be finite and >= 0", k);
        prev = r[k].end;
    }
    if (prev < first + n) return fail(AFR_EINVAL, "optimizer groups: the last range ends at %lld, before the slice's end %lld", (long long)prev, (long long)(first + n));
    tab.n = 0;
    for (int k = 0; k < nr; ++k) {
        if (r[k].end <= first) continue;
        if (tab.n >= AFR_OPT_MAX_RANGES) return fail(AFR_EUNSUPPORTED, "optimizer groups: a slice may cross at most %d ranges", AFR_OPT_MAX_RANGES);
        if (r[k].end / 4 > 0xffffffffll) return fail(AFR_EUNSUPPORTED, "optimizer groups: a flat buffer of 2^34 elements or more");
        const AdamArgs a = group_args(h, r[k]);
        tab.end4[tab.n] = (unsigned)(r[k].end / 4); tab.lr[tab.n] = a.lr; tab.wd[tab.n] = a.wd; tab.step[tab.n] = adam_hyper(a, kind).step;
        tab.n++;
        if (r[k].end >= first + n) break;
    }
    return AFR_OK;
}
// the bf16 weight shadow the GEMMs read / the one a fused optimizer step writes (the same buffer unless the plan has two)
static inline bf16_t* shadow_rd(const afr_plan* p) {
    if (p->cfg.dtype != AFR_BF16) return nullptr;
    return (bf16_t*)(p->ws + ((p->shadow_cur && p->o_shadow2) ? p->o_shadow2 : p->o_shadow));
}
static inline bf16_t* shadow_wr(const afr_plan* p) {
    if (p->cfg.dtype != AFR_BF16) return nullptr;
    if (!p->o_shadow2) return (bf16_t*)(p->ws + p->o_shadow);
    return (bf16_t*)(p->ws + (p->shadow_cur ? p->o_shadow : p->o_shadow2));
}
// the moments the plan's optimizer kind needs are bound (Lion keeps exp_avg only)
static inline bool moments_bound(const afr_plan* p) { return p->M && (p->V || p->opt_kind == OPT_LION); }
// the fused optimizer step of a weight-gradient product: AdamW / Lion on the tensor at flat offset `off`
static void set_fused_opt(const afr_plan* p, GemmParams& g, int64_t off, bf16_t* shadow, const AdamArgs& h) {
    g.ad_p = p->P + off; g.ad_m = p->M + off; g.ad_v = p->opt_kind == OPT_LION ? nullptr : p->V + off;
    g.ad_shadow = shadow ? shadow + off : nullptr;
    g.ad = adam_hyper(args_at(p, h, off), p->opt_kind); g.ad_kind = p->opt_kind;
}
static inline const void* weight_ptr(const afr_plan* p, int64_t off) {
    if (p->cfg.dtype == AFR_BF16) return shadow_rd(p) + off;
    return p->P + off;
}
// The three products of a Linear y[B][N] = x[B][K] . W[N][K]^T + b (gemm.hip) as launch descriptions: M/N/K, the operand
// orientations and dense row-major leading dimensions follow from (B, N, K); `ep` adds epilogue flags.  Whatever else a launch
// carries (row maps, bit masks, fused AdamW, cooperative split-K) the caller sets on the result, by field name.
static inline int out_flag(const afr_plan* p) { return p->cfg.dtype == AFR_BF16 ? AFR_GEMM_OUT_BF16 : 0; }
static GemmParams lin_desc(int flags, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc) {
    GemmParams g;
    g.A = A; g.B = B; g.C = C; g.bias = nullptr; g.aux = nullptr; g.M = M; g.N = N; g.K = K;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldaux = 0; g.flags = flags; g.splitk = 1; g.slab_stride = 0;
    return g;
}
// forward: y = x . W^T + b, in the plan's activation dtype
static GemmParams lin_fwd(const void* x, const void* W, const float* bias, void* y, int B, int N, int K, int ep) {
    GemmParams g = lin_desc(AFR_GEMM_BIAS | ep, x, W, y, B, N, K, K, K, N);
    g.bias = bias;
    return g;
}
static GemmParams lin_fwd(const afr_plan* p, const afr_plan::Layer& l, const void* x, void* y, int B, int ep = 0) {
    return lin_fwd(x, weight_ptr(p, l.w_off), p->P + l.b_off, y, B, l.N, l.K, out_flag(p) | ep);
}
// input gradient: dx = dy . W; aux [B][K] (the layer's input, NULL = none) masks it with ReLU's gate
static GemmParams lin_dx(const void* dy, const void* W, void* dx, const void* aux, int B, int N, int K, int ep) {
    GemmParams g = lin_desc(AFR_GEMM_B_KSTRIDED | (aux ? AFR_GEMM_RELU_MASK : 0) | ep, dy, W, dx, B, K, N, N, K, K);
    g.aux = aux; g.ldaux = aux ? K : 0;
    return g;
}
static GemmParams lin_dx(const afr_plan* p, const afr_plan::Layer& l, const void* dy, void* dx, const void* aux, int B) {
    return lin_dx(dy, weight_ptr(p, l.w_off), dx, aux, B, l.N, l.K, out_flag(p));
}
// weight gradient: dW = dy^T . x with db as the fused column sum; sk > 1: one partial of each per K-slice
static GemmParams lin_dw(const void* dy, const void* x, float* dW, float* db, int B, int N, int K, int sk = 1, long long slab_stride = 0) {
    GemmParams g = lin_desc(AFR_GEMM_A_KSTRIDED | AFR_GEMM_B_KSTRIDED, dy, x, dW, N, K, B, N, K, K);
    g.splitk = sk; g.slab_stride = slab_stride; g.colsum = db; g.colsum_stride = sk > 1 ? N : 0;
    return g;
}
// the bf16 LDS-DMA path addresses an operand with 32-bit byte offsets: 2 GiB per operand
static int check_operand_bytes(const GemmParams& g) {
    const long long ea = (long long)((g.flags & AFR_GEMM_A_KSTRIDED) ? g.K : g.M) * g.lda * 2;
    const long long eb = (long long)((g.flags & AFR_GEMM_B_KSTRIDED) ? g.K : g.N) * g.ldb * 2;
    if (ea < (1ll << 31) && eb < (1ll << 31)) return AFR_OK;
    return fail(AFR_EUNSUPPORTED, "a bf16 GEMM operand must be smaller than 2 GiB (A %lld bytes, B %lld bytes)", ea, eb);
}
// Products collected for ONE grouped launch (a layer's weight gradient + input gradient).  A local of the function that launches
// it: run_gemm collects into the batch it is handed, flush_gemms launches it, an early return simply drops it.
struct GemmBatch {
    static constexpr int MAX = 4;
    int tile256 = 0, n = 0;
    GemmParams g[MAX];
    char tag[MAX][96];
    double fl[MAX] = {0.0, 0.0, 0.0, 0.0}, by[MAX] = {0.0, 0.0, 0.0, 0.0};
    // the cooperative members' Layer::coop_arrived (member 0; a chain's second pair: member 2), advanced once the launch is enqueued
    unsigned* arrived[2] = {nullptr, nullptr};
    // chain: the batch collects TWO layers' pairs (dW_up, dX_up, dW_lo, dX_lo) for one chained launch (afr_launch_gemm_chain)
    bool chain = false;
    // a chain's fifth role (gemm.hip GemmGroup::l1): the folded first layer's fused backward rides the launch; the stage below finds
    // l1_on set and only books the slabs.  l1_loss: the step's deferred loss partials, copied (the descriptor points at it)
    bool l1_on = false; ChainL1 l1; LossSum l1_loss; double l1_fl = 0.0, l1_by = 0.0;
};
static unsigned* l1_cnt_of(const afr_plan* p) { return (unsigned*)(p->ws + p->o_hand) + ((size_t)p->cfg.max_batch + 255) / 256; }
// launches the product, or -- handed a batch, and the product can join a grouped launch -- collects it there
static int run_gemm(afr_plan* p, hipStream_t s, const GemmParams& g, GemmBatch* batch = nullptr) {
    const int gdt = p->gemm_dtype, M = g.M, N = g.N, K = g.K;
    int rc;
    if (gdt == AFR_BF16 && (rc = check_operand_bytes(g))) return rc;
    const double eb = gdt == AFR_BF16 ? 2.0 : 4.0;
    const double ob = (g.flags & AFR_GEMM_OUT_BF16) ? 2.0 : 4.0;
    // algorithmic bytes: operands once + the product once (split-K partial slabs are an implementation choice, not
    // algorithmic output); with the fused optimizer the output is p,m,v read + p,m,v(,shadow) written
    // (Lion: p and m only)
    const double out_bytes = g.ad_p ? (double)M * N * ((g.ad_kind == OPT_LION ? 16.0 : 24.0) + (g.ad_shadow ? 2.0 : 0.0)) : (g.splitk > 1 ? 4.0 : ob) * (double)M * N;
    char tag[96];
    const double fl_ = 2.0 * M * (double)N * K, by_ = eb * ((double)M * K + (double)N * K) + out_bytes;
    {
        const char* kn = afr_gemm_kernel_name(gdt, g);
        if (strcmp(kn, "gemm_bf16_group256") == 0)     // a plain product on the 256x256 body: the operand orientation follows the shape
            snprintf(tag, sizeof tag, "%s[%dx%dx%d]<%d,%d>", kn, M, N, K, (g.flags & AFR_GEMM_A_KSTRIDED) ? 1 : 0, (g.flags & AFR_GEMM_B_KSTRIDED) ? 1 : 0);
        else snprintf(tag, sizeof tag, "%s[%dx%dx%d]", kn, M, N, K);
    }
    const bool joins = batch && afr_gemm_groupable(gdt, g);
    if (g.coop_ws && !(joins && batch->tile256 && (batch->n == 0 || (batch->chain && batch->n == 2))))
        return fail(AFR_ESTATE, "cooperative split-K product outside a 256x256 grouped launch");
    if (g.b_rowmap && !(joins && batch->tile256))
        return fail(AFR_ESTATE, "gathered k-strided operand outside a 256x256 grouped launch");
    if (joins && batch->n < GemmBatch::MAX) {
        batch->g[batch->n] = g; strcpy(batch->tag[batch->n], tag); batch->fl[batch->n] = fl_; batch->by[batch->n] = by_; batch->n++;
        return AFR_OK;
    }
    ProfScope ps(p, s, tag, fl_, by_);
    HIPCHK(afr_launch_gemm(gdt, g, s));
    return AFR_OK;
}
// launch what run_gemm collected: one grouped launch (or the plain one when only one product qualified); members [i0, i0 + n)
static int flush_members(afr_plan* p, hipStream_t s, const GemmBatch& b, int i0, int n, bool chained) {
    if (!n) return AFR_OK;
    char tag[GemmBatch::MAX * 96 + 32];
    int len = snprintf(tag, sizeof tag, "%s", n > 1 ? (b.tile256 ? "gemm_bf16_group256[" : "gemm_bf16_group[") : b.tag[i0]);
    double flops = 0.0, bytes = 0.0;
    for (int i = i0; i < i0 + n && n > 1; ++i) {      // the members' shapes: what stands between the brackets of their tags
        const char* shape = strchr(b.tag[i], '[') + 1;
        len += snprintf(tag + len, sizeof tag - len, "%s%.*s%s", i > i0 ? "+" : "", (int)strcspn(shape, "]"), shape, i == i0 + n - 1 ? "]" : "");
    }
    for (int i = i0; i < i0 + n; ++i) { flops += b.fl[i]; bytes += b.by[i]; }
    const bool l1 = chained && b.l1_on;               // (the row keeps its members' shapes; it gains the first-layer backward's work)
    if (l1) { flops += b.l1_fl; bytes += b.l1_by; }
    hipError_t e;
    const unsigned hand = chained ? p->hand_arrived + afr_gemm_chain_arrivals(b.g) : 0u;
    ChainL1 cl = b.l1;
    if (l1) { cl.cnt = l1_cnt_of(p); cl.target = p->l1_arrived + afr_gemm_chain_l1_arrivals(b.g); if (b.l1_loss.partial) cl.loss = &b.l1_loss; }
    {
        ProfScope ps(p, s, tag, flops, bytes);
        if (chained) e = afr_launch_gemm_chain(p->gemm_dtype, b.g, (unsigned*)(p->ws + p->o_hand), hand, (uint32_t*)(p->ws + p->o_err), s, l1 ? &cl : nullptr);
        else e = afr_launch_gemm_group(p->gemm_dtype, b.g + i0, n, b.tile256, s);
    }
    if (e != hipSuccess) return fail(AFR_EHIP, "grouped GEMM launch: %s", hipGetErrorString(e));
    // the launch carries the cooperative members' arrivals (and a chain's hand-off arrivals): the host counts follow only once
    // it is enqueued
    for (int i = i0; i < i0 + n; i += 2)
        if (b.arrived[i / 2] && b.g[i].coop_ws) *b.arrived[i / 2] = b.g[i].coop_target;
    if (chained) p->hand_arrived = hand;
    if (l1) p->l1_arrived = cl.target;
    return AFR_OK;
}
static int flush_gemms(afr_plan* p, hipStream_t s, GemmBatch& b) {
    if (!b.chain) { b.l1_on = false; return flush_members(p, s, b, 0, b.n, false); }
    // two layers' pairs: ONE chained launch when the launcher takes these descriptors on this device, else the two grouped launches
    // (the first-layer role rides only the chained launch, and only when the launcher takes it: else its own launch follows)
    if (b.n == 4 && p->o_hand && afr_gemm_chain_ok(p->gemm_dtype, b.g)) {
        if (b.l1_on) { ChainL1 t = b.l1; t.cnt = l1_cnt_of(p); b.l1_on = afr_gemm_chain_l1_ok(p->gemm_dtype, b.g, t); }
        return flush_members(p, s, b, 0, 4, true);
    }
    b.l1_on = false;
    if (int rc = flush_members(p, s, b, 0, b.n < 2 ? b.n : 2, false)) return rc;
    return flush_members(p, s, b, 2, b.n > 2 ? b.n - 2 : 0, false);
}
// dW[N][K] = dy[B][N]^T . a[B][K] and db[N] = sum_b dy, reduced over the batch in ONE GEMM launch (the bias gradient
// is the column sum of the A tiles the kernel already stages).  Small outputs use split-K partial slabs, summed later
// by the grouped reduce; large ones (fc_output of the sheet model) write the gradient buffer directly.
static int run_dw(afr_plan* p, hipStream_t s, afr_plan::Layer& l, const void* dy, const void* a, int Bn, RTable& rt, int sk_want = 0,
                  bool coop = false, const int* a_rows = nullptr, int a_ld = 0, GemmBatch* batch = nullptr, StepCtx* step = nullptr) {
    if (a_rows && !coop) return fail(AFR_ESTATE, "gathered weight-gradient operand needs the cooperative 256x256 launch");
    const int N = l.N, K = l.K;
    int sk = sk_want > 0 ? sk_want : choose_splitk(N, K, Bn);
    if (sk > l.sk) sk = l.sk;
    if (sk == 1) return run_gemm(p, s, lin_dw(dy, a, p->G + l.w_off, p->G + l.b_off, Bn, N, K), batch);
    float* sw = (float*)(p->ws + l.o_slab_w);
    float* sb = (float*)(p->ws + l.o_slab_b);
    if (coop) {
        // cooperative split-K: the slices meet inside the launch; the product leaves as the finished gradient, or -- during a
        // fused optimizer step -- as the AdamW update of this weight (its new bf16 copy goes to the write shadow, which the
        // launch's input-gradient workgroups do not read)
        // (each launch adds sk arrivals to every tile's counter; the slices of this one wait for the total after it)
        GemmParams g = lin_dw(dy, a, p->G + l.w_off, sb, Bn, N, K, sk);
        g.coop_ws = sw; g.coop_cnt = (unsigned*)(p->ws + l.o_cnt); g.coop_target = l.coop_arrived + (unsigned)sk;
        g.err = (uint32_t*)(p->ws + p->o_err);
        if (a_rows) { g.b_rowmap = a_rows; g.ldb = a_ld; }      // the layer's input rows are gathered from a table whose rows are a_ld apart
        if (step && step->ndone == AFR_MAX_HIDDEN + 1) return fail(AFR_ESTATE, "more cooperative weight-gradient tails in one step than Linears");
        if (step) set_fused_opt(p, g, l.w_off, shadow_wr(p), step->h);
        int rc = run_gemm(p, s, g, batch);
        if (rc) return rc;
        batch->arrived[(batch->n - 1) / 2] = &l.coop_arrived;      // (batch is non-null: run_gemm refuses a cooperative product it cannot collect)
        if (step) step->done[step->ndone++] = l.w_off;
        afr_rtable_add(rt, p->G + l.b_off, sb, sk, N, N);
        return AFR_OK;
    }
    int rc = run_gemm(p, s, lin_dw(dy, a, sw, sb, Bn, N, K, sk, (long long)N * K), batch);
    if (rc) return rc;
    afr_rtable_add(rt, p->G + l.w_off, sw, sk, (long long)N * K, (long long)N * K);
    afr_rtable_add(rt, p->G + l.b_off, sb, sk, N, N);
    return AFR_OK;
}
static int run_reduce_group(afr_plan* p, hipStream_t s, const RTable& rt, const AdamHyper* seg_ad = nullptr) {
    double bytes = 0;
    for (int i = 0; i < rt.nseg; ++i) bytes += 16.0 * rt.seg[i].n4 * (rt.seg[i].nslabs + 1);
    ProfScope ps(p, s, "reduce_group", 0.0, bytes);
    HIPCHK(afr_launch_reduce_group(rt, s, seg_ad));
    return AFR_OK;
}

extern "C" int afr_sync_params(afr_plan* p, void* stream) {
    if (!p || !p->P) return fail(AFR_ESTATE, "plan has no bound parameters");
    DevGuard dg(p->device);
    p->wT_valid = false;
    if (p->cfg.dtype != AFR_BF16) return AFR_OK;
    HIPCHK(afr_launch_f32_to_bf16(p->P, shadow_rd(p), p->total, (hipStream_t)stream));
    return AFR_OK;
}

// ------------------------------------------------------------------------------------ weight EMA
// while the plan reads its EMA weights (afr_use_ema) nothing may train or step: the gradients, the moments and the step count
// belong to the weights that are parked in p->E meanwhile
static int ema_guard(const afr_plan* p, const char* what) {
    if (p && p->ema_on) return fail(AFR_ESTATE, "%s while the plan reads its EMA weights: afr_use_ema(plan, 0) first", what);
    return AFR_OK;
}
static bool ema_decay_ok(float decay) { return decay > 0.f && decay < 1.f; }      // (false for NaN)
extern "C" int afr_set_ema(afr_plan* p, float* ema, float decay, int every) {
    if (!p) return fail(AFR_EINVAL, "null plan");
    if (int rc = ema_guard(p, "afr_set_ema")) return rc;
    if (!ema) { p->E = nullptr; p->ema_count = 0; return AFR_OK; }
    if (!ema_decay_ok(decay)) return fail(AFR_EINVAL, "the EMA decay must be finite and inside (0, 1), got %g", (double)decay);
    if (every < 1) return fail(AFR_EINVAL, "the EMA interval must be >= 1 optimizer steps, got %d", every);
    if ((uintptr_t)ema & 255) return fail(AFR_EINVAL, "buffers must be 256-byte aligned");
    const int d = device_of(ema);
    if (d >= 0 && p->device >= 0 && d != p->device) return fail(AFR_EINVAL, "the EMA buffer lives on device %d, the plan's buffers on %d", d, p->device);
    p->E = ema; p->ema_decay = decay; p->ema_every = every; p->ema_count = 0;
    return AFR_OK;
}
// one optimizer step has happened: the EMA follows when the interval says so (the plan's own steps and afr_ema_update end here)
static int ema_step(afr_plan* p, const float* sumsq, hipStream_t s) {
    if (!p->E) return AFR_OK;
    if (++p->ema_count % p->ema_every) return AFR_OK;
    ProfScope ps(p, s, "ema", 2.0 * (double)p->total, 12.0 * (double)p->total);
    HIPCHK(afr_launch_ema(p->E, p->P, p->total, p->ema_decay, sumsq, s));
    return AFR_OK;
}
extern "C" int afr_ema_update(afr_plan* p, const float* sumsq_dev, void* stream) {
    if (!p) return fail(AFR_EINVAL, "null plan");
    if (!p->E) return fail(AFR_ESTATE, "no EMA set (afr_set_ema)");
    if (int rc = ema_guard(p, "afr_ema_update")) return rc;
    if (!p->P) return fail(AFR_ESTATE, "plan has no bound parameters");
    DevGuard dg(p->device);
    return ema_step(p, sumsq_dev, (hipStream_t)stream);
}
extern "C" int afr_use_ema(afr_plan* p, int on, void* stream) {
    if (!p) return fail(AFR_EINVAL, "null plan");
    if ((on != 0) == p->ema_on) return AFR_OK;
    if (!p->E) return fail(AFR_ESTATE, "no EMA set (afr_set_ema)");
    if (!p->P || !p->ws) return fail(AFR_ESTATE, "plan has no bound parameters");
    std::swap(p->P, p->E);
    p->ema_on = on != 0;
    p->last.have_du = false; p->last.have_u = false; p->last.next_stage = 0;      // a saved forward belongs to the weights it ran with
    return afr_sync_params(p, stream);          // the bf16 shadow and the transposed copies follow p->P
}
extern "C" int afr_op_ema(float* e, const float* p, int64_t n, float decay, const float* sumsq_dev, void* stream) {
    if (!e || !p) return fail(AFR_EINVAL, "null argument");
    if (n < 0 || (n & 3)) return fail(AFR_EINVAL, "n = %lld must be a non-negative multiple of 4", (long long)n);
    if (!ema_decay_ok(decay)) return fail(AFR_EINVAL, "the EMA decay must be finite and inside (0, 1), got %g", (double)decay);
    DevGuard dg(device_of(e));
    HIPCHK(afr_launch_ema(e, p, n, decay, sumsq_dev, (hipStream_t)stream));
    return AFR_OK;
}

// the dropout description of one pass from the config fields that define it (the plan's, or an afr_op_sheet_* caller's)
static SheetDrop sheet_drop(uint64_t seed, uint64_t step, int rank, float p_embed, float p_attn, float p_fc, int training, float* save) {
    SheetDrop d;
    d.training = training;
    d.key_e = afr_dropout_key(seed, step, AFR_STREAM_EMBED, (uint64_t)rank);
    d.key_a = afr_dropout_key(seed, step, AFR_STREAM_ATTN, (uint64_t)rank);
    d.key_f = afr_dropout_key(seed, step, AFR_STREAM_FC, (uint64_t)rank);
    d.thr_e = afr_keep_threshold(1.f - p_embed);
    d.thr_a = afr_keep_threshold(1.f - p_attn);
    d.thr_f = afr_keep_threshold(1.f - p_fc);
    d.sc_e = 1.f / (1.f - p_embed);
    d.sc_a = 1.f / (1.f - p_attn);
    d.sc_f = 1.f / (1.f - p_fc);
    d.save = save;
    return d;
}
static SheetDrop make_drop(const afr_plan* p, int training, uint64_t step) {
    const afr_config& c = p->cfg;
    // only a training forward leaves o + softmax stats behind
    return sheet_drop(c.seed, step, c.rank, c.p_embed, c.p_attn, c.p_fc, training, training ? (float*)(p->ws + p->o_save) : nullptr);
}
static SheetParams sheet_params(const afr_plan* p) {
    SheetParams sp;
    sp.pos = p->P + p->s_pos; sp.emb = p->P + p->s_emb; sp.w_in = p->P + p->s_win; sp.b_in = p->P + p->s_bin;
    sp.w_o = p->P + p->s_wo; sp.b_o = p->P + p->s_bo; sp.ln_g = p->P + p->s_g; sp.ln_b = p->P + p->s_b;
    sp.w1 = p->P + p->s_w1; sp.b1 = p->P + p->s_b1;
    return sp;
}

// The sheet backward's stage 1 after its dz product: the fused front-end reverse into per-block slabs, registered in rt
static int sheet_front_bwd(afr_plan* p, hipStream_t s, RTable& rt, double flops_per_string) {
    const afr_config& c = p->cfg;
    const int B = p->last.B;
    SheetDims d{p->last.L, c.max_length, c.embed_dim, c.heads, c.fc_dim, c.vocab};
    float* slabs = (float*)(p->ws + p->o_slab_e);
    // a slab is laid out like the flat buffer's first s_wout floats: the 10 small tensors (pos .. fc1.bias)
    SheetSlabOff so{(int)p->s_pos, (int)p->s_emb, (int)p->s_win, (int)p->s_bin, (int)p->s_wo, (int)p->s_bo, (int)p->s_g,
                    (int)p->s_b, (int)p->s_w1, (int)p->s_b1, (int)p->s_wout};
    {
        ProfScope ps(p, s, "sheet_bwd", flops_per_string * B, 0.0);
        HIPCHK(afr_launch_sheet_bwd(c.dtype, d, sheet_params(p), make_drop(p, p->last.training, p->last.step), p->last.x,
                                    p->last.ldx, B, p->ws + p->o_dz, c.ln_eps, slabs, so, s));
    }
    afr_rtable_add(rt, p->G, slabs, afr_sheet_blocks(B), (long long)so.total, (long long)so.total);
    return AFR_OK;
}

// How a glyph layer's gradient pair (dW + dX) leaves at batch B: as ONE grouped launch (sk_group > 0) on 256x256 tiles
// (tile256) with the weight gradient's slices meeting inside the launch (coop), or as separate launches (all zero).
struct PairPlan { int sk_group = 0, tile256 = 0; bool coop = false; };
// what the shape alone allows (afr_op_gemm_pair runs exactly the cooperative ones)
static PairPlan pair_plan_shape(int B, int N, int K) {
    PairPlan pp;
    if (B <= 0 || N < 256 || K <= 0 || (long long)((B + 255) / 256) * ((K + 127) / 128) < 232) return pp;   // (tiles of the input gradient)
    afr_gemm_pair_plan(B, N, K, &pp.tile256, &pp.sk_group);
    // with 256x256 tiles the weight gradient's split-K slices are summed inside the launch (cooperative split-K): no slabs
    // for the grouped reduce to re-read
    pp.coop = pp.tile256 && (pp.sk_group == 2 || pp.sk_group == 4 || pp.sk_group == 8) &&
              (long long)((N + 255) / 256) * ((K + 255) / 256) * pp.sk_group <= 256;
    return pp;
}
static PairPlan pair_plan_for(const afr_plan* p, const afr_plan::Layer& l, int B) {
    const afr_config& c = p->cfg;
    if (c.dtype != AFR_BF16 || (c.reserved & AFR_CFG_NO_GROUPED_GEMM)) return PairPlan();
    PairPlan pp = pair_plan_shape(B, l.N, l.K);
    if (pp.sk_group > l.sk) return PairPlan();                 // the plan's slab space bounds the split
    if (c.reserved & AFR_CFG_SLAB_SPLITK) pp.coop = false;     // keeps the slab path (A/B measurements, parity cross-checks)
    return pp;
}
// The output layer's and the last hidden layer's pairs leave as ONE chained launch (gemm.hip GemmGroup::chain) when both are
// cooperative 256x256 pairs, the block counts of the swapped roles agree and the bound device has a CU per workgroup.  What the
// shapes allow (cus: the device's compute units):
static bool chain_plan_shape(int B, int N_up, int K_up, int K_lo, int cus, PairPlan* up = nullptr, PairPlan* lo = nullptr) {
    const PairPlan pu = pair_plan_shape(B, N_up, K_up), pl = pair_plan_shape(B, K_up, K_lo);
    if (up) *up = pu;
    if (lo) *lo = pl;
    return pu.coop && pl.coop && afr_gemm_chain_counts(B, N_up, K_up, pu.sk_group, K_lo, pl.sk_group, cus, nullptr, nullptr);
}
// ... and what this plan does at batch B (AFR_CFG_NO_PAIR_CHAIN, and every switch that takes a pair off the cooperative body,
// keep the two launches; the hidden layer must be a pair of its own, i.e. not the folded first layer)
static bool chain_for(const afr_plan* p, int B, int cus) {
    const int nl = (int)p->layers.size();
    if (p->cfg.kind != AFR_KIND_GLYPH || nl < 3 || !p->o_hand || (p->cfg.reserved & AFR_CFG_NO_PAIR_CHAIN)) return false;
    const auto &lu = p->layers[nl - 1], &ll = p->layers[nl - 2];
    if (lu.K != ll.N || !pair_plan_for(p, lu, B).coop || !pair_plan_for(p, ll, B).coop) return false;
    return chain_plan_shape(B, lu.N, lu.K, ll.K, cus);
}
extern "C" int afr_plan_pair_chain(const afr_plan* p, int B, int cus) {
    return p && B > 0 && B <= p->cfg.max_batch && chain_for(p, B, cus > 0 ? cus : p->n_cus) ? 1 : 0;
}
// A training forward at batch B runs the first layer as a combination table when every consumer of h1 / h0 can gather: the
// second layer's forward on the 256x128 ring kernel, its gradient pair as a cooperative 256x256 launch, the fused first-layer
// backward.  Decided once per call, before its first launch (decide_step, forward_loss_impl), and handed to forward_impl.
static bool combo_for(const afr_plan* p, int B) {
    if (!p->combo_ok || p->layers.size() < 3) return false;
    const auto& l2 = p->layers[1];
    return afr_gemm_wide_ok(B, l2.N, l2.K) && pair_plan_for(p, l2, B).coop;
}

// ------------------------------------------------------------------------------------- forward
static int forward_impl(afr_plan* p, const int64_t* x, const int64_t* font, int B, int L, float* y, int training,
                        uint64_t step, void* stream, const LossArgs* fl /* the plan's, fused slots */, bool combo = false,
                        LossSum* defer = nullptr /* glyph: the last GEMM only stores its loss partials; *defer = how to add them */) {
    if (!p || !p->P) return fail(AFR_ESTATE, "plan has no bound parameters");
    if (training || fl) if (int rc = ema_guard(p, "a training forward")) return rc;
    DevGuard dg(p->device);
    if (!x) return fail(AFR_EINVAL, "x is null");
    if (B <= 0 || B > p->cfg.max_batch) return fail(AFR_EINVAL, "batch %d outside 1..max_batch=%d", B, p->cfg.max_batch);
    hipStream_t s = (hipStream_t)stream;
    const afr_config& c = p->cfg;
    const int Pix = c.out_h * c.out_w;
    uint32_t* err = (uint32_t*)(p->ws + p->o_err);
    void* u = p->ws + p->o_u;
    int Ldone = 1;      // the length the backward works with: the sheet model's is clipped
    if (c.kind == AFR_KIND_SHEET) {
        if (L <= 0) return fail(AFR_EINVAL, "sequence length must be positive");
        const int Lc = L < c.max_length ? L : c.max_length;               // model.py:163-164
        SheetDims d{Lc, c.max_length, c.embed_dim, c.heads, c.fc_dim, c.vocab};
        void* z = p->ws + p->o_z;
        {
            ProfScope ps(p, s, "sheet_fwd", 2.5e6 * B, 0.0);        // ~2.5 MFLOP of f32 VALU work per string
            HIPCHK(afr_launch_sheet_fwd(c.dtype, d, sheet_params(p), make_drop(p, training, step), x, L, B, z, c.ln_eps, err, s));
        }
        GemmParams g = lin_fwd(p, p->layers[0], z, u, B);        // fc_output
        if (fl) g.loss = *fl;
        int rc = run_gemm(p, s, g);
        if (rc) return rc;
        Ldone = Lc;
    } else if (c.kind == AFR_KIND_PIXEL) {
        // BASELINE configs[4] (oracle.pixel_forward).  Token-wise kernels in pixel.hip, every Linear on the GEMM
        // kernels; the residual stream stays f32; every block keeps what its backward needs (its two residual inputs, LayerNorm
        // outputs, q, k|v, attention output, ReLU output).  No dropout in this model: `training` changes nothing.
        if (c.n_fonts > 0 && !font) return fail(AFR_EINVAL, "font ids are required when n_fonts > 0");
        const int d = c.embed_dim, ff = c.fc_dim, T = Pix, C = c.n_fonts > 0 ? 2 : 1;
        const long long rows = (long long)B * T;
        void *ctx = p->ws + p->o_ctx, *a = p->ws + p->o_a;
        {
            ProfScope ps(p, s, "pixel_ctx", 0.0, 0.0);
            HIPCHK(afr_launch_pixel_ctx(c.dtype, p->P + p->px_emb, p->px_font >= 0 ? p->P + p->px_font : nullptr, x, font, B, d, c.vocab, c.n_fonts, ctx, err, s));
        }
        int rc;
        for (int l = 0; l < c.n_hidden; ++l) {
            const afr_plan::PixBlock& b = p->pix[l];
            const afr_plan::PixSave& sv = p->pxs[l];
            const afr_plan::Layer* L5 = &p->pxl[(size_t)l * 5];           // the block's Linears: q, kv, out-proj, fc1, fc2
            float *hin = (float*)(p->ws + sv.hin), *h1 = (float*)(p->ws + sv.h1);
            void *n1 = p->ws + sv.n1, *q = p->ws + sv.q, *o = p->ws + sv.o, *n2 = p->ws + sv.n2, *kv = p->ws + sv.kv, *f = p->ws + sv.f;
            {
                ProfScope ps(p, s, "pixel_add_ln", 0.0, (double)rows * d * (8.0 + p->act_bytes));
                HIPCHK(afr_launch_pixel_add_ln(c.dtype, l == 0 ? nullptr : (const float*)(p->ws + p->pxs[l - 1].h1), hin, l == 0 ? p->P + p->px_pos : nullptr,
                                               l == 0 ? nullptr : a, p->P + b.ln1g, p->P + b.ln1b, n1, rows, T, d, c.ln_eps, s));
            }
            // packed in-projection (model.py:144): rows [0, d) of in_proj_weight make q from the pixel tokens, rows [d, 3d) k | v from the context
            if ((rc = run_gemm(p, s, lin_fwd(p, L5[0], n1, q, (int)rows)))) return rc;
            if ((rc = run_gemm(p, s, lin_fwd(p, L5[1], ctx, kv, B * C)))) return rc;
            {
                ProfScope ps(p, s, "pixel_attn", 0.0, (double)rows * d * 2.0 * p->act_bytes);
                HIPCHK(afr_launch_pixel_attn(c.dtype, q, kv, o, rows, T, d, c.heads, C, s));
            }
            if ((rc = run_gemm(p, s, lin_fwd(p, L5[2], o, a, (int)rows)))) return rc;
            {
                ProfScope ps(p, s, "pixel_add_ln", 0.0, (double)rows * d * (8.0 + 2.0 * p->act_bytes));
                HIPCHK(afr_launch_pixel_add_ln(c.dtype, hin, h1, nullptr, a, p->P + b.ln2g, p->P + b.ln2b, n2, rows, T, d, c.ln_eps, s));
            }
            // (bf16 mode: the epilogue also leaves the ReLU gate of the stored values as bits for the backward's input-gradient product)
            GemmParams g1 = lin_fwd(p, L5[3], n2, f, (int)rows, AFR_GEMM_RELU);
            if (sv.fbits) { g1.mask_out = (unsigned char*)(p->ws + sv.fbits); g1.ldmask = ff / 8; }
            if ((rc = run_gemm(p, s, g1))) return rc;
            if ((rc = run_gemm(p, s, lin_fwd(p, L5[4], f, a, (int)rows)))) return rc;
        }
        {
            ProfScope ps(p, s, "pixel_head", 0.0, (double)rows * d * (8.0 + p->act_bytes));
            HIPCHK(afr_launch_pixel_head(c.dtype, (const float*)(p->ws + p->pxs.back().h1), (float*)(p->ws + p->o_hf), a, p->P + p->px_lnfg, p->P + p->px_lnfb,
                                         p->P + p->px_wout, p->P + p->px_bout, (float*)u, y, rows, d, c.ln_eps, s, c.loss));
        }
        if (fl) {        // the loss on the f32 pre-clamp output (model.py:156,268-270): du in place over u
            ProfScope ps(p, s, fl->kind == AFR_LOSS_BCE ? "bce_grad" : "mse_grad", 0.0, (double)rows * 9.0);
            HIPCHK(afr_launch_mse_grad(AFR_F32, u, u, B, Pix, loss_slots(*fl, (float*)(p->ws + p->o_loss), false), s));
        }
        p->last.forward_done(x, font, B, 1, L, training, step, fl ? afr_plan::Last::DU : afr_plan::Last::U);
        return AFR_OK;
    } else {
        if (c.n_fonts > 0 && !font) return fail(AFR_EINVAL, "font ids are required when n_fonts > 0");
        void* h = p->ws + p->o_act[0];
        const int nl = (int)p->layers.size();
        const float* femb = c.n_fonts > 0 ? p->P + p->font_off : nullptr;
        int first = 0;
        if (combo) {
            // training step: the first layer as a combination table
            const auto& l = p->layers[0];
            ProfScope ps(p, s, "glyph_l1_combo", 0.0, (double)c.vocab * (c.n_fonts > 0 ? c.n_fonts : 1) * l.N * 2.0);
            HIPCHK(afr_launch_glyph_combo(p->P + p->emb_off, femb, p->P + l.w_off, p->P + l.b_off, x, font, B, c.embed_dim, l.N, c.vocab,
                                          c.n_fonts, (float*)(p->ws + p->o_table), p->ws + p->o_h1c, p->h1c_ld, p->ws + p->o_h0c,
                                          (int*)(p->ws + p->o_cidx), err, s, p->ws + p->o_w1t));
            h = p->ws + p->o_h1c;
            first = 1;
        } else if (p->k0) {
            // hidden layer 1 as a table gather (see glyph_table_kernel); also leaves h0 for the backward dW GEMM
            const auto& l = p->layers[0];
            ProfScope ps(p, s, "glyph_l1_fwd", 0.0, (double)B * l.N * p->act_bytes);
            HIPCHK(afr_launch_glyph_l1_fwd(c.dtype, p->P + p->emb_off, femb, p->P + l.w_off, p->P + l.b_off, x, font, B, c.embed_dim,
                                           l.N, c.vocab, c.n_fonts, (float*)(p->ws + p->o_table), h, p->ws + p->o_act[1], err, s,
                                           p->l1f ? (void*)(p->ws + p->o_w1t) : nullptr));
            h = p->ws + p->o_act[1];
            first = 1;
        } else {
            ProfScope ps(p, s, "glyph_embed", 0.0, 0.0);
            HIPCHK(afr_launch_glyph_embed(c.dtype, p->P + p->emb_off, femb, x, font, B, c.embed_dim, c.vocab, c.n_fonts, h, err, s));
        }
        const bool bits = fl != nullptr && c.dtype == AFR_BF16;
        for (int i = first; i < nl; ++i) {
            const auto& l = p->layers[i];
            const bool last = (i == nl - 1);
            void* outp = last ? u : (void*)(p->ws + p->o_act[i + 1]);
            GemmParams g = lin_fwd(p, l, h, outp, B, last ? 0 : AFR_GEMM_RELU);
            // after the combination table the second layer gathers its input rows from it (rows h1c_ld apart)
            if (combo && i == 1) { g.a_rowmap = (const int*)(p->ws + p->o_cidx); g.lda = p->h1c_ld; }
            if (bits && !last && p->o_mbits[i]) { g.mask_out = (unsigned char*)(p->ws + p->o_mbits[i]); g.ldmask = l.N / 8; }
            if (last && fl) g.loss = *fl;
            if (last && fl && defer) {        // deferred sum: no ticket; tell the caller where the partials are and how they were produced
                g.loss.counter = nullptr;
                defer->partial = fl->partial; defer->inv_n = fl->inv_n; defer->loss_accum = fl->loss_accum;
                afr_gemm_tile_launch_shape(p->gemm_dtype, g, &defer->n, &defer->bd);
            }
            int rc = run_gemm(p, s, g);
            if (rc) return rc;
            h = outp;
        }
    }
    if (y) {
        ProfScope ps(p, s, c.loss == AFR_LOSS_BCE ? "sigmoid_out" : "clamp_out", 0.0, 0.0);
        HIPCHK(afr_launch_clamp_out(c.dtype, u, y, (long long)B * Pix, s, c.loss));
    }
    // (with the loss fused into the last layer's epilogue the buffer already holds du)
    p->last.forward_done(x, font, B, Ldone, L, training, step, fl ? afr_plan::Last::DU : afr_plan::Last::U, combo, c.kind == AFR_KIND_GLYPH && fl && c.dtype == AFR_BF16);
    return AFR_OK;
}
extern "C" int afr_forward(afr_plan* p, const int64_t* x, const int64_t* font, int B, int L, float* y, int training,
                           uint64_t step, void* stream) {
    return forward_impl(p, x, font, B, L, y, training, step, stream, nullptr);
}

// --------------------------------------------------------------------------------- loss + grad
static int check_loss_args(const void* target, int tdtype, int64_t mean_elems, const float* loss_accum) {
    if (!target || !loss_accum) return fail(AFR_EINVAL, "target and loss_accum are required");
    if (tdtype != AFR_TARGET_U8 && tdtype != AFR_TARGET_F32) return fail(AFR_EINVAL, "bad target dtype");
    if (mean_elems <= 0) return fail(AFR_EINVAL, "mean_elems must be positive");
    return AFR_OK;
}
static int loss_grad_impl(afr_plan* p, const void* target, int tdtype, const int* rowmap, int B, int64_t mean_elems, float* loss_accum,
                          void* stream) {
    if (!p || !p->P) return fail(AFR_ESTATE, "plan has no bound parameters");
    DevGuard dg(p->device);
    if (int rc = check_loss_args(target, tdtype, mean_elems, loss_accum)) return rc;
    if (B != p->last.B) return fail(AFR_ESTATE, "loss_grad batch %d does not match the last forward (%d)", B, p->last.B);
    hipStream_t s = (hipStream_t)stream;
    const int Pix = p->cfg.out_h * p->cfg.out_w;
    void* u = p->ws + p->o_u;
    const double tb = tdtype == AFR_TARGET_U8 ? 1.0 : 4.0;
    ProfScope ps(p, s, p->cfg.loss == AFR_LOSS_BCE ? "bce_grad" : "mse_grad", 0.0, (double)B * Pix * (2.0 * p->act_bytes + tb));
    HIPCHK(afr_launch_mse_grad(p->cfg.kind == AFR_KIND_PIXEL ? AFR_F32 : p->cfg.dtype, u, u, B, Pix,      // (the pixel transformer's pre-clamp output is f32 in both modes)
                               loss_args(p, false, target, tdtype, rowmap, mean_elems, loss_accum), s));
    p->last.have_du = true; p->last.have_u = false;
    return AFR_OK;
}
extern "C" int afr_loss_grad(afr_plan* p, const void* target, int tdtype, int B, int64_t mean_elems, float* loss_accum,
                             void* stream) {
    return loss_grad_impl(p, target, tdtype, nullptr, B, mean_elems, loss_accum, stream);
}

// ---------------------------------------------------------------------------------- evaluation
// afr_eval / afr_eval_rows: ONE launch of eval_rows_kernel over the u the last forward saved; u is only read.
static int eval_impl(afr_plan* p, const void* target, int tdtype, const int* rowmap, int B, float* loss_rows, uint32_t* stats, uint8_t* q,
                     void* stream) {
    if (!p || !p->P || !p->ws) return fail(AFR_ESTATE, "plan has no bound parameters");
    if (!loss_rows && !stats && !q) return fail(AFR_EINVAL, "afr_eval: loss_rows, stats and q are all NULL");
    if (!target && (loss_rows || stats)) return fail(AFR_EINVAL, "afr_eval: loss_rows and stats need a target");
    if (target && tdtype != AFR_TARGET_U8 && tdtype != AFR_TARGET_F32) return fail(AFR_EINVAL, "bad target dtype");
    if (B <= 0 || B > p->cfg.max_batch) return fail(AFR_EINVAL, "batch %d outside 1..max_batch=%d", B, p->cfg.max_batch);
    if (((uintptr_t)stats & 15) || ((uintptr_t)q & 7) || ((uintptr_t)loss_rows & 3) || ((uintptr_t)target & (tdtype == AFR_TARGET_U8 ? 7 : 15)))
        return fail(AFR_EINVAL, "afr_eval: stats must be 16-byte aligned, q 8-byte, uint8 targets 8-byte, float32 targets 16-byte");
    if (p->last.B <= 0) return fail(AFR_ESTATE, "afr_eval needs afr_forward first");
    if (B != p->last.B) return fail(AFR_ESTATE, "afr_eval batch %d does not match the last forward (%d)", B, p->last.B);
    if (!p->last.have_u) return fail(AFR_ESTATE, "afr_eval: the output buffer no longer holds u (a loss has written du over it); run afr_forward again");
    DevGuard dg(p->device);
    hipStream_t s = (hipStream_t)stream;
    const int Pix = p->cfg.out_h * p->cfg.out_w;
    const int ad = p->cfg.kind == AFR_KIND_PIXEL ? AFR_F32 : p->cfg.dtype;       // (the pixel transformer's pre-clamp output is f32 in both modes)
    const bool need_t = loss_rows || stats;
    const double bytes = (double)B * Pix * ((ad == AFR_BF16 ? 2.0 : 4.0) + (need_t ? (tdtype == AFR_TARGET_U8 ? 1.0 : 4.0) : 0.0) + (q ? 1.0 : 0.0)) +
                         (double)B * ((loss_rows ? 4.0 : 0.0) + (stats ? 16.0 : 0.0) + (need_t && rowmap ? 4.0 : 0.0));
    ProfScope ps(p, s, "eval_rows", 0.0, bytes);
    HIPCHK(afr_launch_eval_rows(ad, p->cfg.loss, p->ws + p->o_u, target, tdtype, target ? rowmap : nullptr, B, Pix, loss_rows, stats, q, s));
    return AFR_OK;
}
extern "C" int afr_eval(afr_plan* p, const void* target, int tdtype, int B, float* loss_rows, uint32_t* stats, uint8_t* q, void* stream) {
    return eval_impl(p, target, tdtype, nullptr, B, loss_rows, stats, q, stream);
}

extern "C" int afr_set_output_grad(afr_plan* p, const float* dy, int B, void* stream) {
    if (!p || !p->P) return fail(AFR_ESTATE, "plan has no bound parameters");
    DevGuard dg(p->device);
    if (!dy) return fail(AFR_EINVAL, "dy is null");
    if (B != p->last.B) return fail(AFR_ESTATE, "batch %d does not match the last forward (%d)", B, p->last.B);
    HIPCHK(afr_launch_clamp_bwd(p->cfg.kind == AFR_KIND_PIXEL ? AFR_F32 : p->cfg.dtype, p->ws + p->o_u, dy, (long long)B * p->cfg.out_h * p->cfg.out_w, (hipStream_t)stream,
                                p->cfg.loss));
    p->last.have_du = true; p->last.have_u = false;
    return AFR_OK;
}

// ------------------------------------------------------------------------------------ backward
// Backward runs in STAGES, last layer first; each stage finishes a contiguous range of the flat gradient buffer
// (its own slab reduction included), so a data-parallel caller can start the all-reduce of that range while the
// next stage computes.  Glyph: one stage per Linear (the first layer's stage also does the embedding tables).
// Sheet: stage 0 = fc_output (dW + db), stage 1 = dz GEMM + fused front-end backward.  Pixel transformer: one stage per block.

// Backward of the pixel-token transformer (reverse of forward_impl's AFR_KIND_PIXEL branch; oracle.pixel_backward): du (f32,
// left in the u buffer by the loss) -> every parameter gradient.  Linears: the dW (+ fused db) and dX GEMMs of gemm.hip;
// token-wise reverses: pixel.hip.  Slab-produced gradients (split-K dW, bias partials, LayerNorm / head partials) are registered
// for a grouped reduce per block; the rest is written directly.
// One STAGE per block, last block first (stage 0 also runs the head's reverse, the last stage the positional table and the
// embedding rows): each finishes the contiguous range of the flat gradient buffer that holds its block's tensors (stage 0: from
// the last block to the end; the last stage: from the start to the second block), so a data-parallel caller can reduce it while the
// next stage computes.
static int pixel_backward(afr_plan* p, hipStream_t s, int stage, int64_t* g_off, int64_t* g_len) {
    const afr_config& c = p->cfg;
    RTable rt;
    const int B = p->last.B, d = c.embed_dim, ff = c.fc_dim, T = c.out_h * c.out_w, C = c.n_fonts > 0 ? 2 : 1;
    const long long rows = (long long)B * T;
    const int nbp = afr_pixel_bwd_blocks(rows);
    float* du = (float*)(p->ws + p->o_u);
    float* dh = (float*)(p->ws + p->o_dh);
    void* dhT = c.dtype == AFR_BF16 ? (void*)(p->ws + p->o_dht) : (void*)dh;      // the GEMM-operand copy of dh (f32 mode: dh itself)
    void *dfb = p->ws + p->o_df, *dn = p->ws + p->o_dn, *dq = p->ws + p->o_dq, *ctx = p->ws + p->o_ctx;
    int rc;
    const int nl = c.n_hidden, l = nl - 1 - stage;
    if (stage == 0) {
        float* hp = (float*)(p->ws + p->o_headp);
        ProfScope ps(p, s, "pixel_head_bwd", 0.0, (double)rows * d * 12.0);
        HIPCHK(afr_launch_pixel_head_bwd(c.dtype, du, (const float*)(p->ws + p->o_hf), p->P + p->px_lnfg, p->P + p->px_lnfb, p->P + p->px_wout, dh,
                                         c.dtype == AFR_BF16 ? dhT : nullptr, hp, rows, d, c.ln_eps, s));
        afr_rtable_add(rt, p->G + p->px_lnfg, hp, nbp, 4ll * d, d);
        afr_rtable_add(rt, p->G + p->px_lnfb, hp + d, nbp, 4ll * d, d);
        afr_rtable_add(rt, p->G + p->px_wout, hp + 2 * d, nbp, 4ll * d, d);
        afr_rtable_add(rt, p->G + p->px_bout, hp + 3 * d, nbp, 4ll * d, 4);       // (element 0 is db_out; the 3 after it are zero: a 64-aligned tensor)
    }
    {
        const afr_plan::PixBlock& b = p->pix[l];
        const afr_plan::PixSave& sv = p->pxs[l];
        afr_plan::Layer* L5 = &p->pxl[(size_t)l * 5];                 // q, kv, out-proj, fc1, fc2
        // ---- MLP:  h_out = h1 + fc2(relu(fc1(LN2(h1))))
        if ((rc = run_dw(p, s, L5[4], dhT, p->ws + sv.f, (int)rows, rt))) return rc;
        GemmParams g2 = lin_dx(p, L5[4], dhT, dfb, p->ws + sv.f, (int)rows);
        if (sv.fbits) { g2.mask_in = (const unsigned char*)(p->ws + sv.fbits); g2.ldmask = ff / 8; }
        if ((rc = run_gemm(p, s, g2))) return rc;
        if ((rc = run_dw(p, s, L5[3], dfb, p->ws + sv.n2, (int)rows, rt))) return rc;
        if ((rc = run_gemm(p, s, lin_dx(p, L5[3], dfb, dn, nullptr, (int)rows)))) return rc;
        {
            float* lp = (float*)(p->ws + sv.ln2p);
            ProfScope ps(p, s, "pixel_ln_bwd", 0.0, (double)rows * d * (12.0 + 2.0 * p->act_bytes));
            HIPCHK(afr_launch_pixel_ln_bwd(c.dtype, dn, (const float*)(p->ws + sv.h1), p->P + b.ln2g, dh, c.dtype == AFR_BF16 ? dhT : nullptr, lp, rows, d, c.ln_eps, s));
            afr_rtable_add(rt, p->G + b.ln2g, lp, nbp, 2ll * d, d);
            afr_rtable_add(rt, p->G + b.ln2b, lp + d, nbp, 2ll * d, d);
        }
        // ---- attention:  h1 = hin + out_proj(softmax(q k^T) v)
        if ((rc = run_dw(p, s, L5[2], dhT, p->ws + sv.o, (int)rows, rt))) return rc;
        if ((rc = run_gemm(p, s, lin_dx(p, L5[2], dhT, dn, nullptr, (int)rows)))) return rc;
        const int chunk = afr_pixel_attn_chunk(T), chunks = (T + chunk - 1) / chunk;
        float *dkvp = (float*)(p->ws + p->o_dkvp), *dkv = (float*)(p->ws + p->o_dkv);
        {
            ProfScope ps(p, s, "pixel_attn_bwd", 0.0, (double)rows * d * 3.0 * p->act_bytes);
            HIPCHK(afr_launch_pixel_attn_bwd(c.dtype, dn, p->ws + sv.q, p->ws + sv.kv, dq, dkvp, B, T, d, C, s));
        }
        // dk | dv of every context token: the chunk slabs summed in chunk order (one chunk: the kernel's output is the sum)
        if (chunks > 1) {
            ProfScope ps(p, s, "reduce", 0.0, (double)B * 4 * d * 4.0 * (chunks + 1));
            HIPCHK(afr_launch_reduce(dkv, dkvp, chunks, (long long)B * 4 * d, (long long)B * 4 * d, 1.f, 0, s));
        }
        // the GEMM operand [B*C][2d] in the activation dtype: row c of sample b = [dk_c | dv_c] (C = 1: the first 2d of the 4d)
        void* dkvT = p->ws + p->o_dkvt;
        HIPCHK(afr_launch_pixel_cast(c.dtype, dkvT, chunks > 1 ? dkv : dkvp, B, C * 2 * d, 4 * d, s));
        if ((rc = run_dw(p, s, L5[0], dq, p->ws + sv.n1, (int)rows, rt))) return rc;
        if ((rc = run_gemm(p, s, lin_dx(p, L5[0], dq, dn, nullptr, (int)rows)))) return rc;
        if ((rc = run_dw(p, s, L5[1], dkvT, ctx, B * C, rt))) return rc;
        if ((rc = run_gemm(p, s, lin_dx(p, L5[1], dkvT, p->ws + p->o_dctxt, nullptr, B * C)))) return rc;
        HIPCHK(afr_launch_pixel_accum(c.dtype, (float*)(p->ws + p->o_dctx), p->ws + p->o_dctxt, (long long)B * C * d, l == c.n_hidden - 1, s));
        {
            float* lp = (float*)(p->ws + sv.ln1p);
            ProfScope ps(p, s, "pixel_ln_bwd", 0.0, (double)rows * d * (12.0 + 2.0 * p->act_bytes));
            HIPCHK(afr_launch_pixel_ln_bwd(c.dtype, dn, (const float*)(p->ws + sv.hin), p->P + b.ln1g, dh, c.dtype == AFR_BF16 ? dhT : nullptr, lp, rows, d, c.ln_eps, s));
            afr_rtable_add(rt, p->G + b.ln1g, lp, nbp, 2ll * d, d);
            afr_rtable_add(rt, p->G + b.ln1b, lp + d, nbp, 2ll * d, d);
        }
        // a block registers 14 slab sets (5 weights, 5 biases, 4 LayerNorm vectors; + the head's 4 with the last block): summed per
        // block, since the grouped reduce takes 32 segments
        if ((rc = run_reduce_group(p, s, rt))) return rc;
        rt.nseg = 0; rt.nblocks = 0;
    }
    const int64_t lo = l == 0 ? 0 : p->pix[l].ln1g, hi = stage == 0 ? p->total : p->pix[l + 1].ln1g;
    if (g_off) *g_off = lo;
    if (g_len) *g_len = hi - lo;
    if (l > 0) return AFR_OK;
    // positional table: the sum over the batch of the gradient of the residual stream's first value (model.py:140-141 idiom)
    HIPCHK(afr_launch_reduce(p->G + p->px_pos, dh, B, (long long)T * d, (long long)T * d, 1.f, 0, s));
    HIPCHK(afr_launch_pixel_ctx_bwd((const float*)(p->ws + p->o_dctx), p->last.x, p->last.font, B, d, c.vocab, c.n_fonts, p->G + p->px_emb,
                                    p->px_font >= 0 ? p->G + p->px_font : nullptr, s));
    return AFR_OK;
}

// step: the optimizer step this backward is part of (afr_train_step's staged fused path), NULL for a backward on its own
// carry: a caller that runs every stage itself (afr_backward, the staged fused step) lends one GemmBatch to all of them, so that
// stage 0 can leave its pair there for stage 1 to launch both as one chain; NULL (afr_backward_stage: each stage's gradient range
// is final when the call returns, for the caller's all-reduce) keeps a launch per pair.
static int backward_stage_impl(afr_plan* p, int stage, int64_t* g_off, int64_t* g_len, hipStream_t s, RTable* shared_rt, StepCtx* step = nullptr,
                               GemmBatch* carry = nullptr) {
    const afr_config& c = p->cfg;
    const int B = p->last.B;
    void* du = p->ws + p->o_u;
    int rc;
    // slab reductions: flushed per stage (so the stage's gradient range is final), or deferred to ONE grouped launch
    // at the end of a monolithic afr_backward (shared_rt)
    RTable local_rt;
    RTable& rt = shared_rt ? *shared_rt : local_rt;
    auto done = [&](int64_t off, int64_t len) -> int {      // the stage's last step: its slabs summed, its gradient range reported
        if (int r = shared_rt ? AFR_OK : run_reduce_group(p, s, rt)) return r;
        if (g_off) *g_off = off;
        if (g_len) *g_len = len;
        return AFR_OK;
    };
    if (c.kind == AFR_KIND_PIXEL) return pixel_backward(p, s, stage, g_off, g_len);     // (its slab reductions are flushed per stage inside)
    if (c.kind == AFR_KIND_SHEET) {
        if (stage == 0) {
            if ((rc = run_dw(p, s, p->layers[0], du, p->ws + p->o_z, B, rt))) return rc;
            return done(p->s_wout, p->total - p->s_wout);
        }
        if ((rc = run_gemm(p, s, lin_dx(p, p->layers[0], du, p->ws + p->o_dz, nullptr, B)))) return rc;
        if ((rc = sheet_front_bwd(p, s, rt, 7.0e6))) return rc;       // partial recompute + reverse: ~7 MFLOP of f32 work per string
        return done(0, p->s_wout);
    }
    const int nl = (int)p->layers.size();
    const int i = nl - 1 - stage;
    auto& l = p->layers[i];
    const void* a = p->ws + p->o_act[i];
    // d(loss)/d(output of layer i): du for the last layer, else the ping-pong buffer the previous stage wrote
    const void* dy = stage == 0 ? du : (const void*)(p->ws + p->o_d[(stage - 1) & 1]);
    if (i == 0 && p->k0) {
        // folded first layer (glyph_l1_bwd_kernel): ONE weight-gradient GEMM against h0' = [h0 | one-hot] yields dW1, db1
        // and the per-table-row segment sums; a small kernel turns those into dEmb / dFont.  No input-gradient GEMM,
        // no scatter-add.
        const int K0 = p->k0, E = c.embed_dim;
        if (l1_bwd_fused(p)) {
            // throughput mode: one kernel per 64 glyphs (gemm.hip: glyph_l1_bwd_fused_kernel) -> [dW1 | db1 | dTab] slabs
            float* sl = (float*)(p->ws + p->o_l1f);
            const int CS = afr_glyph_l1_bwd_fused_split(B, l.N), nb = afr_glyph_l1_bwd_fused_blocks(B, l.N), nc = l.N / CS;
            const long long st = afr_glyph_l1_bwd_fused_slab_floats(B, l.N, c.vocab, c.n_fonts);
            const bool rode = carry && carry->l1_on && carry->l1.d1 == dy;     // the chained launch above ran it as its fifth role
            if (carry && carry->l1_on && !rode) return fail(AFR_ESTATE, "the chained launch ran the first-layer backward on another d1");
            if (carry) carry->l1_on = false;
            if (!rode) {
                ProfScope ps(p, s, "glyph_l1_bwd_fused", 2.0 * B * l.N * (2.0 * E + 1.0), (double)B * l.N * 2.0 + (double)nb * st * 4.0);
                const LossSum* sum = step ? &step->loss : nullptr;      // the step's deferred loss partials: one more workgroup adds them
                if (p->last.combo_on) HIPCHK(afr_launch_glyph_l1_bwd_fused(dy, l.N, p->ws + p->o_h0c, E, p->ws + p->o_w1t, p->last.x, p->last.font, B, l.N,
                                                                      c.vocab, c.n_fonts, sl, s, (const int*)(p->ws + p->o_cidx), sum));
                else HIPCHK(afr_launch_glyph_l1_bwd_fused(dy, l.N, a, K0, p->ws + p->o_w1t, p->last.x, p->last.font, B, l.N, c.vocab, c.n_fonts, sl, s, nullptr, sum));
            }
            // block = (row block, column range): range cs's slabs are blocks cs, cs + CS, ...; every block has a dTab partial
            for (int cs = 0; cs < CS; ++cs) {
                afr_rtable_add(rt, p->G + l.w_off + (size_t)cs * nc * E, sl + (size_t)cs * st, nb / CS, st * CS, (long long)nc * E);
                afr_rtable_add(rt, p->G + l.b_off + (size_t)cs * nc, sl + (size_t)cs * st + (size_t)nc * E, nb / CS, st * CS, nc);
            }
            afr_rtable_add(rt, p->G + p->emb_off, sl + (size_t)nc * E + nc, nb, st, (long long)c.vocab * E);
            if (c.n_fonts > 0) afr_rtable_add(rt, p->G + p->font_off, sl + (size_t)nc * E + nc + (size_t)c.vocab * E, nb, st, (long long)c.n_fonts * E);
            return done(0, l.b_off + (l.N + 63) / 64 * 64);
        }
        int sk = choose_splitk(l.N, K0, B);
        if (sk > l.sk) sk = l.sk;
        float* sw = (float*)(p->ws + l.o_slab_w);
        float* sb = (float*)(p->ws + l.o_slab_b);
        const long long stride = (long long)l.N * K0;
        if ((rc = run_gemm(p, s, lin_dw(dy, a, sw, sk == 1 ? p->G + l.b_off : sb, B, l.N, K0, sk, sk == 1 ? 0 : stride)))) return rc;
        if (sk > 1) afr_rtable_add(rt, p->G + l.b_off, sb, sk, l.N, l.N);
        float* dw1 = (float*)(p->ws + p->o_dw1);
        float* part = (float*)(p->ws + p->o_slab_e);
        {
            ProfScope ps(p, s, "glyph_l1_bwd", 0.0, (double)sk * l.N * K0 * 4.0);
            HIPCHK(afr_launch_glyph_l1_bwd(sw, sk, stride, p->P + l.w_off, l.N, E, c.vocab, c.n_fonts, dw1, part, s));
        }
        const int nb = afr_glyph_l1_bwd_blocks(l.N);
        const long long pstride = (long long)(c.vocab + c.n_fonts) * E;
        afr_rtable_add(rt, p->G + l.w_off, dw1, 1, 0, (long long)l.N * E);
        afr_rtable_add(rt, p->G + p->emb_off, part, nb, pstride, (long long)c.vocab * E);
        if (c.n_fonts > 0) afr_rtable_add(rt, p->G + p->font_off, part + (size_t)c.vocab * E, nb, pstride, (long long)c.n_fonts * E);
        return done(0, l.b_off + (l.N + 63) / 64 * 64);
    }
    // A layer's two gradient products both consume dy and are independent: when the input-gradient product alone fills the
    // chip with 256x128 tiles they go out as ONE grouped launch, the weight gradient first and split so that one of its
    // blocks runs twice the K-tiles of an input-gradient block (half the slabs of the stand-alone choice; a CU draws
    // either one long block or two short ones).
    const PairPlan pp = pair_plan_for(p, l, B);
    // the layer whose input is the first layer's output: after a combination-table forward its rows are gathered from H1c
    const bool gath = p->last.combo_on && i == 1;
    const int* cidx = gath ? (const int*)(p->ws + p->o_cidx) : nullptr;
    if (gath) {
        if (!pp.coop) return fail(AFR_ESTATE, "combination-table forward without a cooperative gradient pair (batch changed?)");
        a = p->ws + p->o_h1c;
    }
    // a chain: the output layer (stage 0) only collects its pair into the carried batch; the layer below adds its own and launches
    const bool chain_up = carry && stage == 0 && chain_for(p, B, p->n_cus);
    const bool chain_lo = carry && stage == 1 && carry->chain && carry->n == 2;
    if (carry && stage == 1 && carry->chain && !chain_lo) return fail(AFR_ESTATE, "the chained launch lost the output layer's pair");
    GemmBatch local;
    GemmBatch& batch = (chain_up || chain_lo) ? *carry : local;
    if (!chain_lo) { batch = GemmBatch(); batch.tile256 = pp.tile256; batch.chain = chain_up; }
    GemmBatch* const bp = pp.sk_group > 0 ? &batch : nullptr;      // no grouped launch at this shape: each product goes out on its own
    if ((rc = run_dw(p, s, l, dy, a, B, rt, pp.sk_group, pp.coop, cidx, p->h1c_ld, bp, step))) return rc;
    void* dx = p->ws + p->o_d[stage & 1];
    GemmParams g = lin_dx(p, l, dy, dx, i > 0 ? a : nullptr, B);
    if (gath) { g.aux_rowmap = cidx; g.ldaux = p->h1c_ld; }      // the ReLU gate is read from the gathered H1c rows
    if (p->last.mbits_on && i >= 2 && p->o_mbits[i - 1]) { g.mask_in = (const unsigned char*)(p->ws + p->o_mbits[i - 1]); g.ldmask = l.K / 8; }
    if ((rc = run_gemm(p, s, g, bp))) return rc;
    if (chain_lo && i == 1 && p->k0 && l1_bwd_fused(p) && !(c.reserved & AFR_CFG_NO_L1_CHAIN)) {
        // the layer below is the folded first layer and its fused backward reads exactly this dx: it rides the chained launch as a
        // fifth role (the arguments of the stage below, which then only books the slabs).  flush_gemms drops it when the launcher
        // does not take it.
        const auto& l0 = p->layers[0];
        const int E = c.embed_dim, nb1 = afr_glyph_l1_bwd_fused_blocks(B, l0.N);
        ChainL1& d = batch.l1;
        d = ChainL1();
        d.d1 = dx; d.ldd = l0.N; d.W1T = p->ws + p->o_w1t; d.x = p->last.x; d.font = p->last.font; d.B = B; d.N1 = l0.N;
        d.vocab = c.vocab; d.n_fonts = c.n_fonts; d.slabs = (float*)(p->ws + p->o_l1f);
        if (p->last.combo_on) { d.h0 = p->ws + p->o_h0c; d.ldh = E; d.h0_rowmap = (const int*)(p->ws + p->o_cidx); }
        else { d.h0 = p->ws + p->o_act[0]; d.ldh = p->k0; }
        batch.l1_loss = step ? step->loss : LossSum();
        batch.l1_fl = 2.0 * B * l0.N * (2.0 * E + 1.0);
        batch.l1_by = (double)B * l0.N * 2.0 + (double)nb1 * afr_glyph_l1_bwd_fused_slab_floats(B, l0.N, c.vocab, c.n_fonts) * 4.0;
        batch.l1_on = true;
    }
    if (!chain_up && (rc = flush_gemms(p, s, batch))) return rc;
    const int64_t end = l.b_off + (l.N + 63) / 64 * 64;
    if (i > 0) {
        return done(l.w_off, end - l.w_off);
    }
    float* slabs = (float*)(p->ws + p->o_slab_e);
    const int blocks = afr_embed_bwd_blocks(B);
    const long long rows = c.vocab + c.n_fonts;
    {
        ProfScope ps(p, s, "glyph_embed_bwd", 0.0, 0.0);
        HIPCHK(afr_launch_glyph_embed_bwd(c.dtype, dx, p->last.x, p->last.font, B, c.embed_dim, c.vocab, c.n_fonts, slabs, s));
    }
    const long long stride = rows * c.embed_dim;
    afr_rtable_add(rt, p->G + p->emb_off, slabs, blocks, stride, (long long)c.vocab * c.embed_dim);
    if (c.n_fonts > 0)
        afr_rtable_add(rt, p->G + p->font_off, slabs + (size_t)c.vocab * c.embed_dim, blocks, stride, (long long)c.n_fonts * c.embed_dim);
    return done(0, end);
}

extern "C" int afr_backward_stages(const afr_plan* p) {
    if (!p) return 0;
    if (p->cfg.kind == AFR_KIND_PIXEL) return p->cfg.n_hidden;
    return p->cfg.kind == AFR_KIND_SHEET ? 2 : (int)p->layers.size();
}

extern "C" int afr_backward_stage(afr_plan* p, int stage, int64_t* grad_offset, int64_t* grad_elems, void* stream) {
    if (!p || !p->P || !p->G) return fail(AFR_ESTATE, "plan has no bound parameter/gradient buffers");
    if (int rc = ema_guard(p, "afr_backward_stage")) return rc;
    DevGuard dg(p->device);
    const int n = afr_backward_stages(p);
    if (stage < 0 || stage >= n) return fail(AFR_EINVAL, "stage %d outside 0..%d", stage, n - 1);
    if (stage == 0 && !p->last.have_du) return fail(AFR_ESTATE, "backward needs a forward + loss first");
    if (stage != p->last.next_stage) return fail(AFR_ESTATE, "stages must run in order: expected %d, got %d", p->last.next_stage, stage);
    int rc = backward_stage_impl(p, stage, grad_offset, grad_elems, (hipStream_t)stream, nullptr);
    if (rc) return rc;
    p->last.next_stage = stage + 1 == n ? 0 : stage + 1;
    if (stage + 1 == n) p->last.have_du = false;
    return AFR_OK;
}

extern "C" int afr_backward(afr_plan* p, void* stream) {
    if (!p || !p->P || !p->G) return fail(AFR_ESTATE, "plan has no bound parameter/gradient buffers");
    if (int rc = ema_guard(p, "afr_backward")) return rc;
    DevGuard dg(p->device);
    if (!p->last.have_du) return fail(AFR_ESTATE, "afr_backward needs afr_forward + afr_loss_grad first");
    const int n = afr_backward_stages(p);
    RTable rt;
    GemmBatch carry;
    for (int st = 0; st < n; ++st) {
        int rc = backward_stage_impl(p, st, nullptr, nullptr, (hipStream_t)stream, &rt, nullptr, &carry);
        if (rc) return rc;
    }
    int rc = run_reduce_group(p, (hipStream_t)stream, rt);
    if (rc) return rc;
    p->last.next_stage = 0;
    p->last.have_du = false;
    return AFR_OK;
}

// --------------------------------------------------------------------------------------- AdamW
// the sum of squared gradients over the tensor elements inside [lo, hi) of the flat buffer -> *out (device)
static int grad_sumsq_impl(afr_plan* p, int64_t lo, int64_t hi, float* out, float* stats, float gscale, uint32_t* err, hipStream_t s) {
    float* cw = (float*)(p->ws + p->o_clip);
    ProfScope ps(p, s, "grad_sumsq", 2.0 * (double)(hi - lo), 4.0 * (double)(hi - lo));
    HIPCHK(afr_launch_grad_sumsq(p->G, (const SumsqSeg*)(cw + CLIP_WS_TABLE), p->clip_segs.data(), (int)p->clip_segs.size(), lo, hi, cw, out,
                                 stats, gscale, p->clip_norm, err, s));
    return AFR_OK;
}
extern "C" int afr_set_grad_clip(afr_plan* p, float max_norm, float* stats) {
    if (!p) return fail(AFR_EINVAL, "null plan");
    if (!(max_norm >= 0.f) || std::isinf(max_norm)) return fail(AFR_EINVAL, "max_norm must be finite and >= 0 (0 = no clipping), got %g", (double)max_norm);
    p->clip_norm = max_norm;
    p->clip_stats = max_norm > 0.f ? stats : nullptr;
    return AFR_OK;
}
extern "C" int afr_grad_sumsq(afr_plan* p, int64_t offset, int64_t n, float* out, void* stream) {
    if (!p) return fail(AFR_EINVAL, "null plan");
    if ((offset | n) & 3) return fail(AFR_EINVAL, "offset %lld and n %lld must be multiples of 4", (long long)offset, (long long)n);
    if (offset < 0 || n < 0 || offset > p->total || n > p->total - offset)
        return fail(AFR_EINVAL, "range [%lld, +%lld) lies outside the gradient buffer of %lld elements", (long long)offset, (long long)n, (long long)p->total);
    if (!out) return fail(AFR_EINVAL, "out is null");
    if (!p->G || !p->ws) return fail(AFR_ESTATE, "plan has no bound gradient buffer");
    DevGuard dg(p->device);
    return grad_sumsq_impl(p, offset, offset + n, out, nullptr, 1.f, nullptr, (hipStream_t)stream);
}
// ---- per-tensor statistics (include/afr.h): every check first, then elementwise.hip's pair of launches
extern "C" int afr_tensor_stats_chunk(void) { return AFR_TSTATS_CHUNK; }
extern "C" int afr_tensor_stats(afr_plan* p, int which, const float* minus, afr_tensor_stat* out, void* stream) {
    if (!p) return fail(AFR_EINVAL, "null plan");
    if (!out || ((uintptr_t)out & 15)) return fail(AFR_EINVAL, "afr_tensor_stats: out must be a 16-byte aligned device buffer of afr_param_count() records");
    if ((uintptr_t)minus & 15) return fail(AFR_EINVAL, "afr_tensor_stats: minus must be 16-byte aligned");
    const float* a = nullptr;
    const char* what = nullptr;
    switch (which) {
        case AFR_STAT_PARAMS: a = p->P; what = "parameters"; break;
        case AFR_STAT_GRADS: a = p->G; what = "gradients"; break;
        case AFR_STAT_EXP_AVG: a = p->M; what = "exp_avg"; break;
        case AFR_STAT_EXP_AVG_SQ: a = p->V; what = "exp_avg_sq"; break;
        case AFR_STAT_EMA: a = p->E; what = "EMA (afr_set_ema)"; break;
        default: return fail(AFR_EINVAL, "afr_tensor_stats: which must be one of AFR_STAT_* (0..4), got %d", which);
    }
    if (!p->ws) return fail(AFR_ESTATE, "afr_tensor_stats: the plan has no bound buffers (afr_bind)");
    if (!a) return fail(AFR_ESTATE, "afr_tensor_stats: the plan has no %s buffer", what);
    if (!p->tstats_ok) return fail(AFR_EUNSUPPORTED, "afr_tensor_stats: at most %d tensors of fewer than 2^32 elements each", AFR_TSTATS_MAX_SEGS);
    DevGuard dg(p->device);
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(p, s, "tensor_stats", 4.0 * (double)p->total, (minus ? 8.0 : 4.0) * (double)p->total);
    HIPCHK(afr_launch_tensor_stats(a, minus, (const SumsqSeg*)((float*)(p->ws + p->o_clip) + CLIP_WS_TABLE), p->clip_segs.data(), (int)p->clip_segs.size(),
                                   out, (afr_tensor_stat*)(p->ws + p->o_tstats), s));
    return AFR_OK;
}
// the table checks of the op entry: AFR_OK, or the code with the message set
static int tstats_check_segs(const afr_tensor_seg* segs, int nseg) {
    if (nseg < 1 || nseg > AFR_TSTATS_MAX_SEGS) return fail(AFR_EINVAL, "afr_op_tensor_stats: nseg = %d must lie in 1..%d", nseg, AFR_TSTATS_MAX_SEGS);
    if (!segs) return fail(AFR_EINVAL, "afr_op_tensor_stats: segs is null");
    for (int k = 0; k < nseg; ++k) {
        if (segs[k].off < 0 || (segs[k].off & 3)) return fail(AFR_EINVAL, "afr_op_tensor_stats: segs[%d].off = %lld must be a multiple of 4 and >= 0", k, (long long)segs[k].off);
        if (segs[k].numel < 0) return fail(AFR_EINVAL, "afr_op_tensor_stats: segs[%d].numel = %lld is negative", k, (long long)segs[k].numel);
    }
    for (int k = 0; k < nseg; ++k)
        if (segs[k].numel > 0xffffffffll || (segs[k].off >> 2) > 0xffffffffll)
            return fail(AFR_EUNSUPPORTED, "afr_op_tensor_stats: segs[%d] has 2^32 elements or more, or starts at 2^34 or beyond", k);
    return AFR_OK;
}
extern "C" size_t afr_op_tensor_stats_scratch_bytes(const afr_tensor_seg* segs, int nseg) {
    if (tstats_check_segs(segs, nseg)) return 0;
    long long chunks = 0;
    for (int k = 0; k < nseg; ++k) chunks += afr_tstats_seg_blocks(segs[k].numel);
    return (size_t)chunks * sizeof(afr_tensor_stat);
}
extern "C" int afr_op_tensor_stats(const float* a, const float* minus, const afr_tensor_seg* segs, int nseg, afr_tensor_stat* out, void* scratch,
                                   size_t scratch_bytes, void* stream) {
    if (!a || !out || !scratch) return fail(AFR_EINVAL, "afr_op_tensor_stats: a, out and scratch are required");
    if (((uintptr_t)a | (uintptr_t)minus | (uintptr_t)out | (uintptr_t)scratch) & 15) return fail(AFR_EINVAL, "afr_op_tensor_stats: a, minus, out and scratch must be 16-byte aligned");
    if (int rc = tstats_check_segs(segs, nseg)) return rc;
    const size_t need = afr_op_tensor_stats_scratch_bytes(segs, nseg);
    if (scratch_bytes < need) return fail(AFR_EINVAL, "afr_op_tensor_stats: scratch too small: %zu < %zu", scratch_bytes, need);
    SumsqSeg tab[AFR_TSTATS_MAX_SEGS];
    for (int k = 0; k < nseg; ++k) tab[k] = SumsqSeg{(long long)segs[k].off, (long long)segs[k].numel};
    DevGuard dg(device_of(a));
    HIPCHK(afr_launch_tensor_stats(a, minus, nullptr, tab, nseg, out, (afr_tensor_stat*)scratch, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_set_optimizer(afr_plan* p, int kind) {
    if (!p) return fail(AFR_EINVAL, "null plan");
    if (kind != AFR_OPT_ADAMW && kind != AFR_OPT_LION) return fail(AFR_EINVAL, "optimizer kind must be AFR_OPT_ADAMW (0) or AFR_OPT_LION (1), got %d", kind);
    if (int rc = ema_guard(p, "afr_set_optimizer")) return rc;
    p->opt_kind = kind;
    return AFR_OK;
}
extern "C" int afr_set_param_groups(afr_plan* p, const float* lr_mult, const float* wd_mult, int n) {
    if (!p) return fail(AFR_EINVAL, "null plan");
    if (int rc = ema_guard(p, "afr_set_param_groups")) return rc;
    if (n != (int)p->params.size()) return fail(AFR_EINVAL, "afr_set_param_groups: n = %d, the plan has %d parameter tensors", n, (int)p->params.size());
    for (int i = 0; i < n; ++i)
        if ((lr_mult && !mult_ok(lr_mult[i])) || (wd_mult && !mult_ok(wd_mult[i])))
            return fail(AFR_EINVAL, "afr_set_param_groups: the multipliers of tensor %d (%s) must be finite and >= 0", i, p->params[i].name.c_str());
    p->groups.clear();
    if (!lr_mult && !wd_mult) return AFR_OK;
    for (int i = 0; i < n; ++i) {
        const float lm = lr_mult ? lr_mult[i] : 1.f, wm = wd_mult ? wd_mult[i] : 1.f;
        const int64_t end = i + 1 < n ? p->params[i + 1].off : p->total;      // the padding behind a tensor belongs to its range
        if (!p->groups.empty() && p->groups.back().lr_mult == lm && p->groups.back().wd_mult == wm) p->groups.back().end = end;
        else p->groups.push_back(afr_opt_range{end, lm, wm});
    }
    return AFR_OK;
}
extern "C" int afr_param_group_ranges(const afr_plan* p, afr_opt_range* out, int cap) {
    if (!p) return 0;
    const int n = (int)p->groups.size();
    for (int k = 0; out && k < n && k < cap; ++k) out[k] = p->groups[k];
    return n;
}
// The flat update of n elements of caller-owned buffers, ONE launch: every site that steps outside a GEMM or the grouped reduce ends
// here -- the plan's own step, the leftover tensors of a fused step and the afr_op_* optimizer entries.  sumsq: the clipped kernel.
// rg: the slice is [rg->first, rg->first + n) of a flat buffer with these ranges (optimizer groups: the range-aware kernel).
struct FlatRanges { const afr_opt_range* r; int n; int64_t first; };
static int flat_step(int kind, float* P, const float* G, float* M, float* V, bf16_t* shadow, int64_t n, const AdamArgs& h, float gscale, hipStream_t s,
                     const float* sumsq = nullptr, float max_norm = 0.f, const FlatRanges* rg = nullptr) {
    OptRangeTab tab;
    if (rg) if (int rc = build_range_tab(rg->r, rg->n, rg->first, n, h, kind, tab)) return rc;
    HIPCHK(afr_launch_flat_opt(FlatOpt{P, G, M, kind == OPT_LION ? nullptr : V, shadow, n, rg ? rg->first : 0, rg ? &tab : nullptr, h.lr, h.wd,
                                       adam_hyper(h, kind), gscale, sumsq, max_norm, kind}, s));
    return AFR_OK;
}
extern "C" int afr_adamw_step(afr_plan* p, float lr, float b1, float b2, float eps, float wd, int64_t t, float gscale,
                              void* stream) {
    if (!p || !p->P || !p->G || !moments_bound(p))
        return fail(AFR_ESTATE, p && p->opt_kind == OPT_LION ? "Lion needs params, grads and exp_avg bound" : "AdamW needs params, grads and both moments bound");
    if (int rc = ema_guard(p, "an optimizer step")) return rc;
    DevGuard dg(p->device);
    if (int rc = check_step_count(t)) return rc;
    hipStream_t s = (hipStream_t)stream;
    bf16_t* shadow = shadow_rd(p);        // nothing reads the weights concurrently: updated in place
    const float* sumsq = nullptr;
    if (p->clip_norm > 0.f) {             // clipping plan: the global norm first, then the update reads it
        float* cw = (float*)(p->ws + p->o_clip);
        int rc = grad_sumsq_impl(p, 0, p->total, cw + CLIP_WS_SUMSQ, p->clip_stats, gscale, (uint32_t*)(p->ws + p->o_err), s);
        if (rc) return rc;
        sumsq = cw + CLIP_WS_SUMSQ;
    }
    const bool lion = p->opt_kind == OPT_LION, grouped = !p->groups.empty();
    {                                     // the whole buffer in ONE launch (optimizer groups: of the range-aware kernel)
        static const char* const tags[8] = {"adamw", "adamw_clip", "adamw_groups", "adamw_groups_clip", "lion", "lion_clip", "lion_groups", "lion_groups_clip"};
        ProfScope ps(p, s, tags[lion * 4 + grouped * 2 + (sumsq != nullptr)], 0.0, (double)p->total * ((lion ? 20.0 : 28.0) + (shadow ? 2.0 : 0.0)));
        const FlatRanges rg{p->groups.data(), (int)p->groups.size(), 0};
        if (int rc = flat_step(p->opt_kind, p->P, p->G, p->M, p->V, shadow, p->total, AdamArgs{lr, b1, b2, eps, wd, t}, gscale, s, sumsq, p->clip_norm,
                               grouped ? &rg : nullptr)) return rc;
    }
    p->wT_valid = false;
    return ema_step(p, sumsq, s);       // (a skipped step leaves the EMA alone too: the kernel reads the same sum)
}

// Single-GPU optimiser step fused into the grouped slab reduction: every tensor whose gradient was produced as partial
// slabs (split-K dW, bias partials, embedding partials, the sheet model's small tensors) is updated in the kernel that
// sums its slabs -- the summed gradient is never stored; tensors whose gradient a GEMM wrote directly get the plain kernel.
// Optimizer groups: a segment of the grouped reduce is updated with ONE hyper, so a segment that crosses a boundary between two
// ranges (the sheet model's ten small tensors arrive as one) is cut there; the pieces sum the same slabs in the same order.  A
// segment that also keeps a transposed copy cannot be cut (it never spans two tensors): refused, never given one side's scalars.
static int split_segments_at_groups(const afr_plan* p, RTable& rt) {
    RTable nt = rt;
    nt.nseg = 0; nt.nblocks = 0; nt.overflow = 0;
    for (int i = 0; i < rt.nseg; ++i) {
        const RSeg& sg = rt.seg[i];
        const int64_t so = sg.dst - p->G, se = so + sg.n4 * 4;
        for (int64_t cur = so; cur < se;) {
            const int64_t re = range_at(p, cur)->end, pe = re < se ? re : se;
            const bool whole = cur == so && pe == se;
            if (!whole && sg.shT) return fail(AFR_ESTATE, "optimizer groups: a reduce segment with a transposed copy crosses a range boundary at %lld", (long long)re);
            afr_rtable_add(nt, sg.dst + (cur - so), sg.src + (cur - so), sg.nslabs, sg.stride, pe - cur);
            if (whole && !nt.overflow) { RSeg& ns = nt.seg[nt.nseg - 1]; ns.shT = sg.shT; ns.tN = sg.tN; ns.tK = sg.tK; }
            cur = pe;
        }
    }
    if (nt.overflow) return fail(AFR_EUNSUPPORTED, "optimizer groups: the step's reduce segments, cut at the range boundaries, exceed %d", AFR_RT_MAXSEG);
    rt = nt;
    return AFR_OK;
}
static int reduce_and_step(afr_plan* p, hipStream_t s, RTable& rt, const StepCtx& step, int64_t skip_off = -1) {
    const AdamArgs& h = step.h;
    bf16_t* shadow = shadow_wr(p);        // every tensor's new bf16 copy goes to the write shadow; the roles swap below
    const bool lion = p->opt_kind == OPT_LION;
    const bool grouped = !p->groups.empty();
    rt.adam = 1; rt.ad = adam_hyper(h, p->opt_kind); rt.kind = p->opt_kind;
    rt.gbase = p->G; rt.P = p->P; rt.M = p->M; rt.V = lion ? nullptr : p->V; rt.shadow = shadow;
    p->wT_valid = false;
    AdamHyper seg_ad[AFR_RT_MAXSEG];
    int rc;
    if (grouped) {                        // every segment takes the hyper of the range its flat offset lies in
        if (rt.overflow) return fail(AFR_EUNSUPPORTED, "optimizer groups: the step's reduce has more than %d segments", AFR_RT_MAXSEG);
        if ((rc = split_segments_at_groups(p, rt))) return rc;
        for (int i = 0; i < rt.nseg; ++i) seg_ad[i] = adam_hyper(args_at(p, h, rt.seg[i].dst - p->G), p->opt_kind);
    }
    // (an empty table launches nothing either way: the launcher returns before it looks at the hypers)
    rc = run_reduce_group(p, s, rt, grouped ? seg_ad : nullptr);
    if (rc) return rc;
    for (const Tensor& tn : p->params) {
        if (tn.off == skip_off) continue;
        bool done = false;                 // updated inside its weight-gradient GEMM (cooperative split-K tail)
        for (int k = 0; k < step.ndone; ++k) done = done || step.done[k] == tn.off;
        if (done) continue;
        // covered by the (disjoint) segments of the grouped reduce -- possibly several per tensor (column ranges)?
        int64_t cov = 0;
        for (int i = 0; i < rt.nseg; ++i) {
            const int64_t so = rt.seg[i].dst - p->G, se = so + rt.seg[i].n4 * 4;
            const int64_t lo = so > tn.off ? so : tn.off, hi = se < tn.off + tn.numel ? se : tn.off + tn.numel;
            if (hi > lo) cov += hi - lo;
        }
        if (cov >= tn.numel) continue;
        const int64_t n = (tn.numel + 63) / 64 * 64;
        ProfScope ps(p, s, lion ? "lion" : "adamw", 0.0, (double)n * (lion ? 20.0 : 28.0));
        if ((rc = flat_step(p->opt_kind, p->P + tn.off, p->G + tn.off, p->M + tn.off, lion ? nullptr : p->V + tn.off, shadow ? shadow + tn.off : nullptr, n,
                            args_at(p, h, tn.off), 1.f, s))) return rc;
    }
    if (p->o_shadow2) p->shadow_cur ^= 1;   // every tensor has been rewritten: the write shadow is the current one now
    return ema_step(p, nullptr, s);         // the step's last parameter write is behind us (never a clipping plan here)
}

// Single-GPU sheet step with the optimizer fused into the weight-gradient GEMM: fc_output.weight (99.98 % of the
// parameters) gets its AdamW update in the epilogue of dW = du^T.z, tile by tile, so its gradient is never written to
// or re-read from HBM (-8 bytes/parameter/step) and the update traffic overlaps other tiles' MFMA work.  dz = du.W
// runs FIRST because it must see the pre-update weights.  The small tensors take the ordinary AdamW kernel.
static bool fused_step_eligible(const afr_plan* p, int B) {      // (the model and the shape; decide_step adds the rest)
    return p->cfg.kind == AFR_KIND_SHEET && choose_splitk(p->layers[0].N, p->layers[0].K, B) == 1;
}
static int sheet_fused_step(afr_plan* p, hipStream_t s, const StepCtx& step) {
    const afr_plan::Layer& l = p->layers[0];      // fc_output
    const int B = p->last.B;
    void* du = p->ws + p->o_u;
    bf16_t* shadow = shadow_rd(p);        // the sheet model keeps ONE shadow: its input-gradient product runs before the update
    int rc;
    if ((rc = run_gemm(p, s, lin_dx(p, l, du, p->ws + p->o_dz, nullptr, B)))) return rc;
    GemmParams g = lin_dw(du, p->ws + p->o_z, p->G + l.w_off, p->G + l.b_off, B, l.N, l.K);
    set_fused_opt(p, g, l.w_off, shadow, step.h);
    if ((rc = run_gemm(p, s, g))) return rc;
    RTable rt;
    if ((rc = sheet_front_bwd(p, s, rt, 9.0e6))) return rc;
    // the ten small tensors are updated inside the slab reduction; fc_output.bias by the plain kernel; fc_output.weight
    // was updated in the dW GEMM above (skipped here)
    if ((rc = reduce_and_step(p, s, rt, step, l.w_off))) return rc;
    p->last.have_du = false;
    p->last.next_stage = 0;
    return AFR_OK;
}

// One fused launch for the whole forward + loss + backward of a small one-hidden-layer glyph net (glyph_fused.hip); the
// per-block partial gradients it leaves are registered in `rt` for the grouped reduce (with or without AdamW).
static int glyph1_fused(afr_plan* p, const int64_t* x, const int64_t* font, const void* target, int tdtype, const int* rowmap, int B,
                        int64_t mean_elems, float* loss_accum, hipStream_t s, RTable& rt) {
    const afr_config& c = p->cfg;
    if (!x) return fail(AFR_EINVAL, "x is null");
    if (B <= 0 || B > c.max_batch) return fail(AFR_EINVAL, "batch %d outside 1..max_batch=%d", B, c.max_batch);
    if (c.n_fonts > 0 && !font) return fail(AFR_EINVAL, "font ids are required when n_fonts > 0");
    const auto& l1 = p->layers[0];
    const auto& l2 = p->layers[1];
    const int E = c.embed_dim, N1 = l1.N, Pix = l2.N;
    const bool b16 = c.dtype == AFR_BF16;
    if (b16 && !p->wT_valid) {
        ProfScope ps(p, s, "glyph1_transpose", 0.0, 0.0);
        HIPCHK(afr_launch_transpose_bf16(p->P + l1.w_off, (bf16_t*)(p->ws + p->o_w1t), N1, E, s));
        HIPCHK(afr_launch_transpose_bf16(p->P + l2.w_off, (bf16_t*)(p->ws + p->o_w2t), Pix, N1, s));
        p->wT_valid = true;
    }
    Glyph1Args a;
    a.x = x; a.font = font; a.loss = loss_args(p, true, target, tdtype, rowmap, mean_elems, loss_accum);
    a.B = B; a.E = E; a.N1 = N1; a.P = Pix; a.vocab = c.vocab; a.n_fonts = c.n_fonts;
    a.emb = p->P + p->emb_off; a.femb = c.n_fonts > 0 ? p->P + p->font_off : nullptr;
    a.b1 = p->P + l1.b_off; a.b2 = p->P + l2.b_off;
    a.W1 = weight_ptr(p, l1.w_off); a.W2 = weight_ptr(p, l2.w_off);
    a.W1T = b16 ? (const void*)(p->ws + p->o_w1t) : (const void*)(p->P + l1.w_off);
    a.W2T = b16 ? (const void*)(p->ws + p->o_w2t) : (const void*)(p->P + l2.w_off);
    a.slabs = (float*)(p->ws + p->o_slab1); a.slab_stride = p->total;
    a.o_emb = p->emb_off; a.o_font = c.n_fonts > 0 ? p->font_off : 0; a.o_w1 = l1.w_off; a.o_b1 = l1.b_off; a.o_w2 = l2.w_off; a.o_b2 = l2.b_off;
    a.err = (uint32_t*)(p->ws + p->o_err);
    const int R = afr_glyph1_rows(c.dtype), nrb = (B + R - 1) / R, cs = afr_glyph1_colsplit(c.dtype, B, Pix), nblk = nrb * cs;
    a.cs = cs;
    {
        const double fl = 6.0 * B * ((double)E * N1 + (double)N1 * Pix);
        ProfScope ps(p, s, b16 ? "glyph1_step<bf16>" : "glyph1_step<f32>", fl, (double)nblk * p->total * 4.0 + (double)B * Pix);
        HIPCHK(afr_launch_glyph1_step(c.dtype, a, s));
    }
    for (const Tensor& tn : p->params) {
        if (cs > 1 && (tn.off == l2.w_off || tn.off == l2.b_off)) {
            // fc_output's rows are split over the cs blocks of a row block: block (rb, pc) holds rows [pc, pc + 1) * Pix / cs, so
            // each row range is its own segment over the slabs rb * cs + pc
            const long long per = tn.off == l2.w_off ? (long long)(Pix / cs) * N1 : Pix / cs;
            for (int pc = 0; pc < cs; ++pc) {
                afr_rtable_add(rt, p->G + tn.off + pc * per, a.slabs + (size_t)pc * p->total + tn.off + pc * per, nrb, (long long)cs * p->total, per);
                if (b16 && tn.off == l2.w_off && rt.nseg > 0 && !rt.overflow) {
                    RSeg& sg = rt.seg[rt.nseg - 1];
                    sg.shT = (bf16_t*)(p->ws + p->o_w2t) + (size_t)pc * (Pix / cs); sg.tN = Pix; sg.tK = N1;      // columns pc * Pix / cs .. of W2^T [N1][Pix]
                }
            }
            continue;
        }
        afr_rtable_add(rt, p->G + tn.off, a.slabs + tn.off, nblk, p->total, (tn.numel + 3) / 4 * 4);
        // when the optimizer runs inside this reduce, it also keeps the transposed operand copies current
        if (b16 && rt.nseg > 0 && !rt.overflow) {
            RSeg& sg = rt.seg[rt.nseg - 1];
            if (tn.off == l1.w_off) { sg.shT = (bf16_t*)(p->ws + p->o_w1t); sg.tN = N1; sg.tK = E; }
            if (tn.off == l2.w_off) { sg.shT = (bf16_t*)(p->ws + p->o_w2t); sg.tN = Pix; sg.tK = N1; }
        }
    }
    p->last.forward_done(x, font, B, /*L*/ 1, /*ldx*/ 1, /*training*/ 1, /*step*/ 0, afr_plan::Last::NOTHING);      // (nothing for a backward or an evaluation: the step is complete)
    return AFR_OK;
}

static int forward_loss_impl(afr_plan* p, const int64_t* x, const int64_t* font, const void* target, int tdtype, const int* rowmap, int B, int L,
                             int64_t mean_elems, float* loss_accum, uint64_t step, void* stream) {
    if (int rc = check_loss_args(target, tdtype, mean_elems, loss_accum)) return rc;
    const LossArgs fl = loss_args(p, true, target, tdtype, rowmap, mean_elems, loss_accum);
    return forward_impl(p, x, font, B, L, nullptr, 1, step, stream, &fl, combo_for(p, B));
}
extern "C" int afr_forward_loss(afr_plan* p, const int64_t* x, const int64_t* font, const void* target, int tdtype, int B, int L,
                                int64_t mean_elems, float* loss_accum, uint64_t step, void* stream) {
    return forward_loss_impl(p, x, font, target, tdtype, nullptr, B, L, mean_elems, loss_accum, step, stream);
}

// ---- the way a training step goes: decided ONCE per call, before its first launch
enum StepPath {
    STEP_GLYPH1,          // small one-hidden-layer glyph net: forward + loss + backward in ONE launch, then the grouped reduce
    STEP_SHEET_FUSED,     // sheet model: fc_output.weight is stepped inside its weight-gradient GEMM (sheet_fused_step)
    STEP_STAGED_FUSED,    // the staged backward as one pass that carries the step (StepCtx), then reduce_and_step
    STEP_UNFUSED          // afr_backward materialises every gradient, then afr_adamw_step when the call steps
};
// fuse_opt: the optimizer runs inside the path's own launches (GLYPH1: inside its grouped reduce); combo: combo_for
struct StepPlan { StepPath path; bool fuse_opt, defer_loss, combo; };
// Refuses (nothing enqueued, the plan unchanged) or fills `d` from the bound buffers, the optimizer and clipping settings, cfg.reserved
static int decide_step(const afr_plan* p, int B, int do_step, int64_t t, StepPlan& d) {
    if (!p->G) return fail(AFR_ESTATE, "plan has no bound gradient buffer");
    if (do_step) if (int rc = check_step_count(t)) return rc;
    const auto rs = p->cfg.reserved;
    // (a clipping plan needs the global norm before any update: every gradient is materialised, then afr_adamw_step)
    const bool fuse = do_step && !(rs & AFR_CFG_UNFUSED_OPTIMIZER) && !(p->clip_norm > 0.f) && moments_bound(p);
    d = StepPlan{STEP_GLYPH1, fuse, false, false};
    if (p->fused1 && !(rs & AFR_CFG_NO_FUSED_GLYPH1)) return AFR_OK;
    d.path = !fuse ? STEP_UNFUSED : fused_step_eligible(p, B) ? STEP_SHEET_FUSED : p->cfg.kind != AFR_KIND_PIXEL ? STEP_STAGED_FUSED : STEP_UNFUSED;
    d.fuse_opt = d.path != STEP_UNFUSED;
    // When the call runs the whole backward and the step itself and the first-layer backward is the fused kernel, nothing before
    // the end of the step reads the loss: the forward's last GEMM only stores its partials (no ticket, no last-block sum at the
    // end of that launch) and one workgroup appended to the first-layer backward's grid adds them -- the same arithmetic, bit for
    // bit.  Every other path keeps the ticket.
    d.defer_loss = d.path == STEP_STAGED_FUSED && l1_bwd_fused(p) && p->gemm_dtype == AFR_BF16;
    d.combo = combo_for(p, B);
    return AFR_OK;
}
static int train_step_impl(afr_plan* p, const int64_t* x, const int64_t* font, const void* target, int tdtype, const int* rowmap, int B,
                           int L, int64_t mean_elems, float* loss_accum, uint64_t step, int do_step, float lr, float b1,
                           float b2, float eps, float wd, int64_t t, void* stream) {
    int rc;
    if ((rc = check_loss_args(target, tdtype, mean_elems, loss_accum))) return rc;
    if (!p || !p->P) return fail(AFR_ESTATE, "plan has no bound parameters");
    if ((rc = ema_guard(p, "afr_train_step"))) return rc;
    StepPlan d;
    if ((rc = decide_step(p, B, do_step, t, d))) return rc;
    DevGuard dg(p->device);
    hipStream_t s = (hipStream_t)stream;
    StepCtx sc{AdamArgs{lr, b1, b2, eps, wd, t}};
    RTable rt;
    if (d.path != STEP_GLYPH1) {
        // the loss and its gradient are computed in the epilogue of the last forward GEMM: u never touches HBM
        const LossArgs fl = loss_args(p, true, target, tdtype, rowmap, mean_elems, loss_accum);
        if ((rc = forward_impl(p, x, font, B, L, nullptr, 1, step, stream, &fl, d.combo, d.defer_loss ? &sc.loss : nullptr))) return rc;
    }
    switch (d.path) {
    case STEP_GLYPH1:
        if ((rc = glyph1_fused(p, x, font, target, tdtype, rowmap, B, mean_elems, loss_accum, s, rt))) return rc;
        if (d.fuse_opt) {
            rc = reduce_and_step(p, s, rt, sc);
            p->wT_valid = rc == AFR_OK;                 // the reduce's AdamW wrote W1T / W2T beside the shadow
            return rc;
        }
        if ((rc = run_reduce_group(p, s, rt))) return rc;
        break;
    case STEP_SHEET_FUSED:
        return sheet_fused_step(p, s, sc);
    case STEP_STAGED_FUSED:
        // weight-gradient products with a cooperative split-K tail apply this step's AdamW themselves
    {
        GemmBatch carry;
        for (int st = 0, n = afr_backward_stages(p); st < n; ++st)
            if ((rc = backward_stage_impl(p, st, nullptr, nullptr, s, &rt, &sc, &carry))) return rc;
    }
        p->last.next_stage = 0; p->last.have_du = false;
        return reduce_and_step(p, s, rt, sc);
    case STEP_UNFUSED:
        if ((rc = afr_backward(p, stream))) return rc;
        break;
    }
    return do_step ? afr_adamw_step(p, lr, b1, b2, eps, wd, t, 1.f, stream) : AFR_OK;
}
extern "C" int afr_train_step(afr_plan* p, const int64_t* x, const int64_t* font, const void* target, int tdtype, int B,
                              int L, int64_t mean_elems, float* loss_accum, uint64_t step, int do_step, float lr, float b1,
                              float b2, float eps, float wd, int64_t t, void* stream) {
    return train_step_impl(p, x, font, target, tdtype, nullptr, B, L, mean_elems, loss_accum, step, do_step, lr, b1, b2, eps, wd, t, stream);
}

// ------------------------------------------------------------------- resident data set, by row index
// The afr_*_rows entry points are the dense ones with (x, font, target) taken from the bound data set at rows[b]: the targets
// through the loss kernels' row maps (read in place), codes and font ids through the workspace staging that
// dataset_rows_kernel fills -- which is what last_x / last_font then name, so the backward entry points need nothing new.
extern "C" int afr_bind_dataset(afr_plan* p, const int64_t* x, const int64_t* font, const void* target, int tdtype, int64_t n_rows, int L) {
    if (!p) return fail(AFR_EINVAL, "null plan");
    if (!x && !font && !target) {
        p->ds_x = p->ds_font = nullptr; p->ds_target = nullptr; p->ds_rows = 0; p->ds_L = 0;
        return AFR_OK;
    }
    if (n_rows >= (1ll << 31)) return fail(AFR_EUNSUPPORTED, "a data set of %lld rows: row indices are narrowed to 32 bits (fewer than 2^31 rows)", (long long)n_rows);
    if (!x || !target || n_rows <= 0) return fail(AFR_EINVAL, "a data set needs codes, targets and at least one row");
    if (p->cfg.n_fonts > 0 && !font) return fail(AFR_EINVAL, "font ids are required when n_fonts > 0");
    if (L <= 0 || (p->cfg.kind != AFR_KIND_SHEET && L != 1)) return fail(AFR_EINVAL, "bad row length L = %d (sheet: positive; glyph / pixel: 1)", L);
    if (tdtype != AFR_TARGET_U8 && tdtype != AFR_TARGET_F32) return fail(AFR_EINVAL, "bad target dtype");
    p->ds_x = x; p->ds_font = p->cfg.n_fonts > 0 ? font : nullptr; p->ds_target = target; p->ds_tdtype = tdtype; p->ds_rows = n_rows; p->ds_L = L;
    return AFR_OK;
}
// the checks every afr_*_rows call starts with, then (stage_ids) the prepare kernel; *Lc = the staged row length
static int rows_begin(afr_plan* p, const int64_t* rows, int B, bool stage_ids, void* stream, int* Lc) {
    if (!p || !p->ds_target) return fail(AFR_ESTATE, "no data set bound (afr_bind_dataset)");
    if (!rows) return fail(AFR_EINVAL, "rows is null");
    if (B <= 0 || B > p->cfg.max_batch) return fail(AFR_EINVAL, "batch %d outside 1..max_batch=%d", B, p->cfg.max_batch);
    if (!p->P || !p->ws) return fail(AFR_ESTATE, "plan has no bound parameters");
    DevGuard dg(p->device);
    hipStream_t s = (hipStream_t)stream;
    *Lc = p->cfg.kind == AFR_KIND_SHEET ? (p->ds_L < p->cfg.max_length ? p->ds_L : p->cfg.max_length) : 1;
    ProfScope ps(p, s, "dataset_rows", 0.0, (double)B * (stage_ids ? 16.0 * *Lc + 28.0 : 12.0));
    HIPCHK(afr_launch_dataset_rows(rows, B, p->ds_rows, p->ds_x, p->ds_font, p->ds_L, *Lc, (int*)(p->ws + p->o_ridx),
                                   stage_ids ? (int64_t*)(p->ws + p->o_sx) : nullptr, (int64_t*)(p->ws + p->o_sfont), (uint32_t*)(p->ws + p->o_err), s));
    return AFR_OK;
}
static inline const int64_t* staged_font(const afr_plan* p) { return p->ds_font ? (const int64_t*)(p->ws + p->o_sfont) : nullptr; }
extern "C" int afr_forward_rows(afr_plan* p, const int64_t* rows, int B, float* y, int training, uint64_t step, void* stream) {
    int Lc, rc;
    if (training && (rc = ema_guard(p, "a training forward"))) return rc;
    if ((rc = rows_begin(p, rows, B, true, stream, &Lc))) return rc;
    return forward_impl(p, (const int64_t*)(p->ws + p->o_sx), staged_font(p), B, Lc, y, training, step, stream, nullptr);
}
extern "C" int afr_loss_grad_rows(afr_plan* p, const int64_t* rows, int B, int64_t mean_elems, float* loss_accum, void* stream) {
    int Lc, rc;      // (the row indices alone: the staged codes of the forward stay as they are for the backward)
    if ((rc = rows_begin(p, rows, B, false, stream, &Lc))) return rc;
    return loss_grad_impl(p, p->ds_target, p->ds_tdtype, (const int*)(p->ws + p->o_ridx), B, mean_elems, loss_accum, stream);
}
extern "C" int afr_eval_rows(afr_plan* p, const int64_t* rows, int B, float* loss_rows, uint32_t* stats, uint8_t* q, void* stream) {
    int Lc, rc;      // (the row indices alone, as afr_loss_grad_rows: the kernel reads the targets where they lie)
    if (!loss_rows && !stats && !q) return fail(AFR_EINVAL, "afr_eval_rows: loss_rows, stats and q are all NULL");
    if ((rc = rows_begin(p, rows, B, false, stream, &Lc))) return rc;
    return eval_impl(p, p->ds_target, p->ds_tdtype, (const int*)(p->ws + p->o_ridx), B, loss_rows, stats, q, stream);
}
extern "C" int afr_forward_loss_rows(afr_plan* p, const int64_t* rows, int B, int64_t mean_elems, float* loss_accum, uint64_t step,
                                     void* stream) {
    int Lc, rc;
    if ((rc = ema_guard(p, "afr_forward_loss_rows"))) return rc;
    if ((rc = rows_begin(p, rows, B, true, stream, &Lc))) return rc;
    return forward_loss_impl(p, (const int64_t*)(p->ws + p->o_sx), staged_font(p), p->ds_target, p->ds_tdtype, (const int*)(p->ws + p->o_ridx),
                             B, Lc, mean_elems, loss_accum, step, stream);
}
extern "C" int afr_train_step_rows(afr_plan* p, const int64_t* rows, int B, int64_t mean_elems, float* loss_accum, uint64_t step,
                                   int do_step, float lr, float b1, float b2, float eps, float wd, int64_t t, void* stream) {
    int Lc, rc;
    if ((rc = ema_guard(p, "afr_train_step_rows"))) return rc;
    // the loss arguments and the step count before the staging kernel: a step refused for them enqueues nothing
    if (p && p->ds_target && (rc = check_loss_args(p->ds_target, p->ds_tdtype, mean_elems, loss_accum))) return rc;
    if (do_step && (rc = check_step_count(t))) return rc;
    if ((rc = rows_begin(p, rows, B, true, stream, &Lc))) return rc;
    return train_step_impl(p, (const int64_t*)(p->ws + p->o_sx), staged_font(p), p->ds_target, p->ds_tdtype, (const int*)(p->ws + p->o_ridx),
                           B, Lc, mean_elems, loss_accum, step, do_step, lr, b1, b2, eps, wd, t, stream);
}

extern "C" int afr_error_flags(afr_plan* p, void* stream, uint32_t* out) {
    if (!p || !p->ws || !out) return fail(AFR_EINVAL, "plan must be bound and out non-null");
    DevGuard dg(p->device);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(out, p->ws + p->o_err, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (*out) HIPCHK(hipMemsetAsync(p->ws + p->o_err, 0, sizeof(uint32_t), s));   // read-and-clear
    return AFR_OK;
}

extern "C" int afr_debug_copy(afr_plan* p, int which, void* dst, size_t cap, size_t* bytes_out, void* stream) {
    if (!p || !p->ws || !dst) return fail(AFR_EINVAL, "plan must be bound and dst non-null");
    DevGuard dg(p->device);
    if (p->last.B <= 0) return fail(AFR_ESTATE, "no forward has run yet");
    const afr_config& c = p->cfg;
    const size_t B = (size_t)p->last.B, ab = (size_t)p->act_bytes;
    size_t off = 0, bytes = 0;
    if (which == AFR_BUF_U) { off = p->o_u; bytes = B * c.out_h * c.out_w * ab; }
    else if (which == AFR_BUF_Z && c.kind == AFR_KIND_SHEET) { off = p->o_z; bytes = B * c.max_length * c.fc_dim * ab; }
    else if (which == AFR_BUF_DZ && c.kind == AFR_KIND_SHEET) { off = p->o_dz; bytes = B * c.max_length * c.fc_dim * ab; }
    else if ((which == AFR_BUF_W1T || which == AFR_BUF_W2T) && p->fused1 && c.dtype == AFR_BF16) {
        const int N1 = p->layers[0].N, Pix = p->layers[1].N;
        off = which == AFR_BUF_W1T ? p->o_w1t : p->o_w2t;
        bytes = (size_t)(which == AFR_BUF_W1T ? c.embed_dim * N1 : N1 * Pix) * 2;
    }
    else if (which >= AFR_BUF_ACT && c.kind == AFR_KIND_GLYPH && which - AFR_BUF_ACT < (int)p->o_act.size()) {
        const int i = which - AFR_BUF_ACT;
        off = p->o_act[i];
        bytes = B * (size_t)(i == 0 ? (p->k0 ? p->k0 : c.embed_dim) : c.hidden[i - 1]) * ab;
    } else if (which >= AFR_BUF_ACT && c.kind == AFR_KIND_PIXEL && which - AFR_BUF_ACT < (int)p->pxs.size()) {
        off = p->pxs[which - AFR_BUF_ACT].f;           // block i's ReLU output f [B * tokens][fc_dim]: its sign is the MLP's gate
        bytes = B * (size_t)c.out_h * c.out_w * c.fc_dim * ab;
    } else return fail(AFR_EINVAL, "no such buffer %d for this model kind", which);
    if (bytes > cap) return fail(AFR_EINVAL, "destination too small: %zu < %zu", cap, bytes);
    HIPCHK(hipMemcpyAsync(dst, p->ws + off, bytes, hipMemcpyDefault, (hipStream_t)stream));
    if (bytes_out) *bytes_out = bytes;
    return AFR_OK;
}

extern "C" int afr_debug_sheet_gather(afr_plan* p, const int64_t* x, int B, int L, float* e0, void* stream) {
    if (!p || !p->P || !p->ws) return fail(AFR_ESTATE, "plan has no bound parameters");
    if (p->cfg.kind != AFR_KIND_SHEET) return fail(AFR_EINVAL, "the sheet model's gather: plan is not AFR_KIND_SHEET");
    if (!x || !e0) return fail(AFR_EINVAL, "x and e0 are required");
    if (B <= 0 || B > p->cfg.max_batch || L <= 0) return fail(AFR_EINVAL, "batch %d / length %d out of range", B, L);
    DevGuard dg(p->device);
    const afr_config& c = p->cfg;
    const int Lc = L < c.max_length ? L : c.max_length;
    SheetDims d{Lc, c.max_length, c.embed_dim, c.heads, c.fc_dim, c.vocab};
    SheetDrop dr = make_drop(p, 0, 0);
    dr.dbg_e0 = e0;
    HIPCHK(afr_launch_sheet_fwd(c.dtype, d, sheet_params(p), dr, x, L, B, p->ws + p->o_z, c.ln_eps, (uint32_t*)(p->ws + p->o_err),
                                (hipStream_t)stream));
    p->last.have_du = false;
    return AFR_OK;
}

// --------------------------------------------------------------------------- single-kernel ops
extern "C" int afr_op_gemm(int dtype, int flags, const void* A, const void* B, void* C, const float* bias, const void* aux,
                           int M, int N, int K, int lda, int ldb, int ldc, int ldaux, int splitk, void* stream) {
    if (!A || !B || !C) return fail(AFR_EINVAL, "null operand");
    if (M <= 0 || N <= 0 || K <= 0 || splitk < 1) return fail(AFR_EINVAL, "bad GEMM extents");
    if (dtype != AFR_F32 && dtype != AFR_BF16 && dtype != AFR_BF16X3) return fail(AFR_EINVAL, "dtype must be AFR_F32, AFR_BF16 or AFR_BF16X3");
    if (dtype == AFR_BF16X3 && (flags & AFR_GEMM_OUT_BF16)) return fail(AFR_EINVAL, "AFR_BF16X3 products have an f32 output (no AFR_GEMM_OUT_BF16)");
    const int v = dtype == AFR_BF16 ? 8 : 4;
    const bool ak = flags & AFR_GEMM_A_KSTRIDED, bk = flags & AFR_GEMM_B_KSTRIDED;
    if ((ak ? M : K) % v || (bk ? N : K) % v || lda % v || ldb % v || N % v || ldc % v)
        return fail(AFR_EUNSUPPORTED, "contiguous extents and leading dimensions must be multiples of %d", v);
    if (splitk > 1 && (flags & (AFR_GEMM_BIAS | AFR_GEMM_RELU | AFR_GEMM_RELU_MASK | AFR_GEMM_OUT_BF16)))
        return fail(AFR_EINVAL, "split-K output is plain f32 partial slabs");
    GemmParams g;
    g.A = A; g.B = B; g.C = C; g.bias = bias; g.aux = aux; g.M = M; g.N = N; g.K = K;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldaux = ldaux; g.flags = flags; g.splitk = splitk;
    g.slab_stride = (long long)M * ldc;
    int rc;
    if (dtype == AFR_BF16 && (rc = check_operand_bytes(g))) return rc;
    DevGuard dg(device_of(C));
    HIPCHK(afr_launch_gemm(dtype, g, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" size_t afr_op_gemm_fix_workspace_bytes(int M, int N, int head_tiles, int splitk) {
    const long long tiles = (long long)((M + 255) / 256) * ((N + 255) / 256);
    const long long tail = tiles - (head_tiles < tiles ? (head_tiles < 0 ? 0 : head_tiles) : tiles);
    return (size_t)(tail * splitk) * AFR_FIX_SLICE_BYTES + (size_t)(tail > 0 ? tail : 1) * sizeof(unsigned);
}
extern "C" int afr_op_gemm_fix(int flags, const void* A, const void* B, void* C, const float* bias, const void* aux,
                               int M, int N, int K, int lda, int ldb, int ldc, int ldaux, int head_tiles, int splitk,
                               void* workspace, size_t workspace_bytes, void* stream) {
    if (!A || !B || !C || !workspace) return fail(AFR_EINVAL, "null operand");
    if (M <= 0 || N <= 0 || K <= 0 || splitk < 1 || splitk > 64 || head_tiles < 0) return fail(AFR_EINVAL, "bad GEMM extents");
    const bool ak = flags & AFR_GEMM_A_KSTRIDED, bk = flags & AFR_GEMM_B_KSTRIDED;
    if ((ak ? M : K) % 8 || (bk ? N : K) % 8 || lda % 8 || ldb % 8 || N % 8 || ldc % 8)
        return fail(AFR_EUNSUPPORTED, "contiguous extents and leading dimensions must be multiples of 8");
    GemmParams g;
    g.A = A; g.B = B; g.C = C; g.bias = bias; g.aux = aux; g.M = M; g.N = N; g.K = K;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldaux = ldaux; g.flags = flags; g.splitk = splitk;
    if (int rc = check_operand_bytes(g)) return rc;
    const size_t need = afr_op_gemm_fix_workspace_bytes(M, N, head_tiles, splitk);
    if (workspace_bytes < need || ((uintptr_t)workspace & 15)) return fail(AFR_EINVAL, "workspace too small or misaligned: %zu < %zu", workspace_bytes, need);
    const long long tiles = (long long)((M + 255) / 256) * ((N + 255) / 256);
    const long long tail = tiles - (head_tiles < tiles ? head_tiles : tiles);
    DevGuard dg(device_of(C));
    g.head_tiles = head_tiles;
    g.fix_ws = (float*)workspace;
    g.fix_cnt = (unsigned*)((char*)workspace + (size_t)(tail * splitk) * AFR_FIX_SLICE_BYTES);
    HIPCHK(afr_launch_gemm_fix(g, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_gemm_pair_plan(int B, int N, int K, int* splitk, size_t* workspace_bytes) {
    const PairPlan pp = pair_plan_shape(B, N, K);
    const int sk = pp.sk_group;
    if (!pp.coop) return fail(AFR_EUNSUPPORTED, "%d x %d x %d does not run as a cooperative 256x256 pair", B, N, K);
    const size_t tiles = (size_t)((N + 255) / 256) * ((K + 255) / 256);
    if (splitk) *splitk = sk;
    if (workspace_bytes) *workspace_bytes = tiles * sk * AFR_FIX_SLICE_BYTES + align_up(tiles * sizeof(unsigned), 256);
    return AFR_OK;
}
extern "C" int afr_op_gemm_pair(const void* dy, const void* x, const void* W, const void* aux, float* dW, float* db_part, void* dX,
                                int B, int N, int K, void* workspace, size_t workspace_bytes, void* stream) {
    if (!dy || !x || !W || !dW || !db_part || !dX || !workspace) return fail(AFR_EINVAL, "null operand");
    int sk; size_t need;
    int rc = afr_op_gemm_pair_plan(B, N, K, &sk, &need);
    if (rc) return rc;
    if (N % 8 || K % 8) return fail(AFR_EUNSUPPORTED, "N and K must be multiples of 8");
    if (workspace_bytes < need || ((uintptr_t)workspace & 255)) return fail(AFR_EINVAL, "workspace too small or misaligned: %zu < %zu", workspace_bytes, need);
    GemmParams g[2] = {lin_dw(dy, x, dW, db_part, B, N, K, sk), lin_dx(dy, W, dX, aux, B, N, K, AFR_GEMM_OUT_BF16)};
    if ((rc = check_operand_bytes(g[0])) || (rc = check_operand_bytes(g[1]))) return rc;
    DevGuard dg(device_of(dW));
    hipStream_t s = (hipStream_t)stream;
    const size_t tiles = (size_t)((N + 255) / 256) * ((K + 255) / 256);
    unsigned* cnt = (unsigned*)((char*)workspace + tiles * sk * AFR_FIX_SLICE_BYTES);
    HIPCHK(hipMemsetAsync(cnt, 0, align_up(tiles * sizeof(unsigned), 256), s));
    g[0].coop_ws = (float*)workspace; g[0].coop_cnt = cnt; g[0].coop_target = (unsigned)sk;
    HIPCHK(afr_launch_gemm_group(AFR_BF16, g, 2, 1, s));
    return AFR_OK;
}
// ---- afr_op_linear: one product of a Linear as the step issues it (lin_fwd / lin_dx / lin_dw + the tails, set by name)
static size_t pair_workspace_bytes(int N, int K, const PairPlan& pp) {
    if (!pp.coop) return 0;
    const size_t tiles = (size_t)((N + 255) / 256) * ((K + 255) / 256);
    return tiles * pp.sk_group * AFR_FIX_SLICE_BYTES + align_up(tiles * sizeof(unsigned), 256);
}
extern "C" int afr_op_linear_pair_plan(int B, int N, int K, int* tile256, int* splitk, int* coop, size_t* workspace_bytes) {
    const PairPlan pp = pair_plan_shape(B, N, K);
    if (pp.sk_group < 1) return fail(AFR_EUNSUPPORTED, "%d x %d x %d: the gradient pair does not leave as one grouped launch", B, N, K);
    if (tile256) *tile256 = pp.tile256;
    if (splitk) *splitk = pp.sk_group;
    if (coop) *coop = pp.coop ? 1 : 0;
    if (workspace_bytes) *workspace_bytes = pair_workspace_bytes(N, K, pp);
    return AFR_OK;
}
// a launcher's answer: what it refuses (hipErrorInvalidValue before anything is launched) is a refusal, not a HIP failure
static int launcher_rc(hipError_t e, const char* what) {
    if (e == hipSuccess) return AFR_OK;
    (void)hipGetLastError();
    if (e == hipErrorInvalidValue)
        return fail(AFR_EUNSUPPORTED, "afr_op_linear (%s): the GEMM launcher refuses this combination of dtype, operand layout, shape and tails", what);
    return fail(AFR_EHIP, "afr_op_linear (%s): %s", what, hipGetErrorString(e));
}
// the ReLU gates of an input-gradient product (aux / aux_rows / mask_in), as backward_stage_impl sets them
static int linear_set_gate(GemmParams& g, const afr_linear_tail& t, int dtype, int K) {
    if (t.aux_rows && !t.aux) return fail(AFR_EINVAL, "aux_rows without aux");
    if (t.ldaux && t.ldaux < K && !t.aux_rows) return fail(AFR_EINVAL, "ldaux = %d is smaller than K = %d", t.ldaux, K);
    if (t.ldaux % (dtype == AFR_BF16 ? 8 : 4)) return fail(AFR_EUNSUPPORTED, "ldaux must be a multiple of %d", dtype == AFR_BF16 ? 8 : 4);
    if (t.aux && t.ldaux) g.ldaux = t.ldaux;
    if (t.aux_rows) g.aux_rowmap = t.aux_rows;
    if (t.mask_in) {
        if (dtype != AFR_BF16) return fail(AFR_EINVAL, "mask_in: bit masks exist with bf16 outputs only");
        if (t.ldmask < K / 8) return fail(AFR_EINVAL, "ldmask = %d is smaller than K / 8 = %d", t.ldmask, K / 8);
        g.flags |= AFR_GEMM_RELU_MASK; g.mask_in = t.mask_in; g.ldmask = t.ldmask;
    }
    return AFR_OK;
}
// the fused optimizer step of a weight-gradient product, as set_fused_opt sets it
static int linear_set_opt(GemmParams& g, const afr_linear_tail& t, int dtype) {
    if (!t.p) return AFR_OK;
    if (t.shadow && dtype != AFR_BF16) return fail(AFR_EINVAL, "fused optimizer: the bf16 shadow exists in AFR_BF16 only");
    if (t.opt_kind != AFR_OPT_ADAMW && t.opt_kind != AFR_OPT_LION) return fail(AFR_EINVAL, "optimizer kind must be AFR_OPT_ADAMW (0) or AFR_OPT_LION (1), got %d", t.opt_kind);
    if (!t.m || (t.opt_kind == AFR_OPT_ADAMW && !t.v)) return fail(AFR_EINVAL, "fused optimizer: null moment");
    if (int rc = check_step_count(t.t)) return rc;
    if (t.grad_scale != 1.f) return fail(AFR_EUNSUPPORTED, "fused optimizer: the GEMM tails take the gradient unscaled (grad_scale must be 1, got %g)", (double)t.grad_scale);
    g.ad_p = t.p; g.ad_m = t.m; g.ad_v = t.opt_kind == AFR_OPT_LION ? nullptr : t.v; g.ad_shadow = (bf16_t*)t.shadow;
    g.ad = adam_hyper(AdamArgs{t.lr, t.beta1, t.beta2, t.eps, t.weight_decay, t.t}, t.opt_kind); g.ad_kind = t.opt_kind;
    return AFR_OK;
}
// the two members of AFR_LIN_PAIR as backward_stage_impl builds them (g[0] = dW, g[1] = dx); a cooperative pair's counters are zeroed on s
static int linear_pair_members(int dtype, const afr_linear_tail& t, const void* x, const void* W, const void* dy, void* out, void* out2,
                               int B, int N, int K, int ldo, int ldx, int ld_db, void* workspace, size_t workspace_bytes, hipStream_t s,
                               GemmParams* g, PairPlan* plan) {
    int rc;
    const PairPlan pp = pair_plan_shape(B, N, K);
    const int sk = pp.sk_group;
    if (sk < 1) return fail(AFR_EUNSUPPORTED, "%d x %d x %d: the gradient pair does not leave as one grouped launch", B, N, K);
    if (!t.db) return fail(AFR_EINVAL, "AFR_LIN_PAIR: db is required");
    if (t.x_rows && !pp.coop) return fail(AFR_EUNSUPPORTED, "a gathered weight-gradient operand needs the cooperative 256x256 launch");
    if (t.p && !pp.coop) return fail(AFR_EUNSUPPORTED, "a fused optimizer step inside a grouped launch needs the cooperative 256x256 launch");
    g[0] = lin_dw(dy, x, (float*)out, t.db, B, N, K, sk, pp.coop ? 0 : (long long)N * ldo);
    g[0].ldc = ldo; g[0].ldb = ldx; g[0].colsum_stride = ld_db;
    if (t.x_rows) g[0].b_rowmap = t.x_rows;
    if ((rc = linear_set_opt(g[0], t, dtype))) return rc;
    g[1] = lin_dx(dy, W, out2, t.aux, B, N, K, AFR_GEMM_OUT_BF16);
    g[1].ldc = ldo;      // (both members are [.][K]: one ld_out serves dW / p / m / v and dx)
    if ((rc = linear_set_gate(g[1], t, dtype, K))) return rc;
    if (pp.coop) {
        const size_t need = pair_workspace_bytes(N, K, pp);
        if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 255)) return fail(AFR_EINVAL, "workspace missing, too small or misaligned: %zu < %zu", workspace_bytes, need);
        const size_t tiles = (size_t)((N + 255) / 256) * ((K + 255) / 256);
        unsigned* cnt = (unsigned*)((char*)workspace + tiles * sk * AFR_FIX_SLICE_BYTES);
        HIPCHK(hipMemsetAsync(cnt, 0, align_up(tiles * sizeof(unsigned), 256), s));
        g[0].coop_ws = (float*)workspace; g[0].coop_cnt = cnt; g[0].coop_target = (unsigned)sk;
    }
    // (the grouped launcher would answer a member that cannot join with separate launches: here that is a refusal)
    if (!afr_gemm_groupable(dtype, g[0]) || !afr_gemm_groupable(dtype, g[1]))
        return fail(AFR_EUNSUPPORTED, "%d x %d x %d: a member of the pair cannot join a grouped launch", B, N, K);
    if ((rc = check_operand_bytes(g[0])) || (rc = check_operand_bytes(g[1]))) return rc;
    *plan = pp;
    return AFR_OK;
}
extern "C" int afr_op_linear(int dtype, int which, const void* x, const void* W, const float* bias, const void* dy, void* out, void* out2,
                             int B, int N, int K, const afr_linear_tail* tail, void* workspace, size_t workspace_bytes,
                             char* kernel_name, int name_cap, void* stream) {
    static const afr_linear_tail none = {};
    const afr_linear_tail& t = tail ? *tail : none;
    if (dtype != AFR_F32 && dtype != AFR_BF16 && dtype != AFR_BF16X3) return fail(AFR_EINVAL, "dtype must be AFR_F32, AFR_BF16 or AFR_BF16X3");
    if (which < AFR_LIN_FWD || which > AFR_LIN_PAIR) return fail(AFR_EINVAL, "which must be AFR_LIN_FWD, _DX, _DW or _PAIR");
    if (B <= 0 || N <= 0 || K <= 0) return fail(AFR_EINVAL, "bad Linear extents %d x %d x %d", B, N, K);
    if (!out) return fail(AFR_EINVAL, "null output");
    const bool fwd = which == AFR_LIN_FWD, dx = which == AFR_LIN_DX, dw = which == AFR_LIN_DW, pair = which == AFR_LIN_PAIR;
    if (fwd ? (!x || !W || !bias) : dx ? (!dy || !W) : dw ? (!dy || !x) : (!dy || !x || !W || !out2)) return fail(AFR_EINVAL, "null operand");
    if (kernel_name && name_cap < 1) return fail(AFR_EINVAL, "name_cap must be positive");
    // a tail the product does not have is an error, not something to drop
    if (!fwd && (t.target || t.target_rows || t.mask_out)) return fail(AFR_EINVAL, "the fused loss and mask_out belong to AFR_LIN_FWD");
    if ((fwd || dw) && (t.aux || t.aux_rows || t.mask_in)) return fail(AFR_EINVAL, "aux, aux_rows and mask_in belong to AFR_LIN_DX / AFR_LIN_PAIR");
    if ((fwd || dx) && (t.db || t.p || t.splitk > 1)) return fail(AFR_EINVAL, "db, splitk and the fused optimizer belong to AFR_LIN_DW / AFR_LIN_PAIR");
    if (dx && t.x_rows) return fail(AFR_EINVAL, "x_rows belongs to AFR_LIN_FWD / AFR_LIN_PAIR");
    if (dw && t.x_rows) return fail(AFR_EUNSUPPORTED, "a gathered weight-gradient operand needs the cooperative 256x256 launch (AFR_LIN_PAIR)");
    const int v = dtype == AFR_BF16 ? 8 : 4;
    const int out_w = (fwd ? N : K), ldo = t.ld_out ? t.ld_out : out_w, ldx = t.ldx ? t.ldx : K, ld_db = t.ld_db ? t.ld_db : N;
    if (N % v || K % v || ldo % v || ldx % v) return fail(AFR_EUNSUPPORTED, "N, K and the leading dimensions must be multiples of %d", v);
    if (ldo < out_w || ldx < K || ld_db < N || t.splitk < 0) return fail(AFR_EINVAL, "a leading dimension is smaller than its row, or splitk < 0");
    if (pair && dtype != AFR_BF16) return fail(AFR_EUNSUPPORTED, "AFR_LIN_PAIR: grouped launches exist in AFR_BF16 only");
    const int ob = dtype == AFR_BF16 ? AFR_GEMM_OUT_BF16 : 0;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    DevGuard dg(device_of(out));
    GemmParams g[2];
    if (fwd) {
        g[0] = lin_fwd(x, W, bias, out, B, N, K, ob | (t.mask_out ? AFR_GEMM_RELU : 0));
        g[0].ldc = ldo;
        if (t.target) {
            if ((rc = check_loss_args(t.target, t.target_dtype, t.mean_elems, t.loss_accum))) return rc;
            if (t.loss_kind != AFR_LOSS_MSE && t.loss_kind != AFR_LOSS_BCE) return fail(AFR_EINVAL, "loss kind must be AFR_LOSS_MSE (0) or AFR_LOSS_BCE (1), got %d", t.loss_kind);
            if (!t.loss_scratch) return fail(AFR_EINVAL, "fused loss: null scratch");
            if (t.mask_out) return fail(AFR_EINVAL, "the fused loss belongs to the last layer, mask_out to a hidden one");
            g[0].loss = loss_args(t.loss_scratch, true, t.loss_kind, t.target, t.target_dtype, t.target_rows, t.mean_elems, t.loss_accum);
        } else if (t.target_rows) return fail(AFR_EINVAL, "target_rows without target");
        if (t.mask_out) {
            if (dtype != AFR_BF16) return fail(AFR_EINVAL, "mask_out: bit masks exist with bf16 outputs only");
            if (t.ldmask < N / 8) return fail(AFR_EINVAL, "ldmask = %d is smaller than N / 8 = %d", t.ldmask, N / 8);
            g[0].mask_out = t.mask_out; g[0].ldmask = t.ldmask;
        }
        g[0].lda = ldx;
        if (t.x_rows) g[0].a_rowmap = t.x_rows;
    } else if (dx) {
        g[0] = lin_dx(dy, W, out, t.aux, B, N, K, ob);
        g[0].ldc = ldo;
        if ((rc = linear_set_gate(g[0], t, dtype, K))) return rc;
    } else if (dw) {
        const int sk = t.splitk > 1 ? t.splitk : 1;
        if (sk > 1 && t.p) return fail(AFR_EINVAL, "the fused optimizer step takes the whole gradient: splitk must be 1 (the cooperative pair splits inside its launch)");
        g[0] = lin_dw(dy, x, (float*)out, t.db, B, N, K, sk, sk > 1 ? (long long)N * ldo : 0);
        g[0].ldc = ldo; g[0].ldb = ldx;
        if (t.db && sk > 1) g[0].colsum_stride = ld_db;
        if ((rc = linear_set_opt(g[0], t, dtype))) return rc;
    } else {
        PairPlan pp;
        if ((rc = linear_pair_members(dtype, t, x, W, dy, out, out2, B, N, K, ldo, ldx, ld_db, workspace, workspace_bytes, s, g, &pp))) return rc;
        if ((rc = launcher_rc(afr_launch_gemm_group(dtype, g, 2, pp.tile256, s), "pair"))) return rc;
        if (kernel_name) snprintf(kernel_name, name_cap, "%s", !pp.tile256 ? "gemm_bf16_group" : (t.p && t.opt_kind == AFR_OPT_LION) ? "gemm_bf16_group256_lion" : "gemm_bf16_group256");
        return AFR_OK;
    }
    if (dtype == AFR_BF16 && (rc = check_operand_bytes(g[0]))) return rc;
    if ((rc = launcher_rc(afr_launch_gemm(dtype, g[0], s), fwd ? "forward" : dx ? "input gradient" : "weight gradient"))) return rc;
    if (kernel_name) snprintf(kernel_name, name_cap, "%s", afr_gemm_kernel_name(dtype, g[0]));
    return AFR_OK;
}
// ---- afr_op_linear_chain: two stacked Linears' pairs as the one chained launch of a glyph step (afr_launch_gemm_chain)
static int chain_cus(int cus) {
    if (cus > 0) return cus;
    int d = 0, n = 0;
    if (hipGetDevice(&d) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}
extern "C" int afr_op_linear_chain_plan(int B, int N_up, int K_up, int K_lo, int cus, int* splitk_up, int* splitk_lo, int* blocks, size_t* workspace_bytes) {
    PairPlan pu, pl;
    if (!chain_plan_shape(B, N_up, K_up, K_lo, chain_cus(cus), &pu, &pl))
        return fail(AFR_EUNSUPPORTED, "%d x (%d x %d over %d x %d): the two gradient pairs do not leave as one chained launch", B, N_up, K_up, K_up, K_lo);
    int front = 0, back = 0;
    afr_gemm_chain_counts(B, N_up, K_up, pu.sk_group, K_lo, pl.sk_group, 1 << 30, &front, &back);
    if (splitk_up) *splitk_up = pu.sk_group;
    if (splitk_lo) *splitk_lo = pl.sk_group;
    if (blocks) *blocks = 2 * (front + back);
    if (workspace_bytes) *workspace_bytes = pair_workspace_bytes(N_up, K_up, pu) + pair_workspace_bytes(K_up, K_lo, pl) + align_up(((size_t)B + 255) / 256 * sizeof(unsigned), 256);
    return AFR_OK;
}
// the four products' shapes alone, in chain order (what the block map reads)
static void chain_shapes(int B, int N_up, int K_up, int K_lo, const PairPlan& pu, const PairPlan& pl, GemmParams* g) {
    g[0] = lin_dw(nullptr, nullptr, nullptr, nullptr, B, N_up, K_up, pu.sk_group);
    g[1] = lin_dx(nullptr, nullptr, nullptr, nullptr, B, N_up, K_up, AFR_GEMM_OUT_BF16);
    g[2] = lin_dw(nullptr, nullptr, nullptr, nullptr, B, K_up, K_lo, pl.sk_group);
    g[3] = lin_dx(nullptr, nullptr, nullptr, nullptr, B, K_up, K_lo, AFR_GEMM_OUT_BF16);
}
extern "C" int afr_op_linear_chain_block(int B, int N_up, int K_up, int K_lo, int block, int* phase, int* member, int* tm, int* tn, int* slice) {
    PairPlan pu, pl;
    if (!phase || !member || !tm || !tn || !slice) return fail(AFR_EINVAL, "null output");
    if (!chain_plan_shape(B, N_up, K_up, K_lo, 1 << 30, &pu, &pl))
        return fail(AFR_EUNSUPPORTED, "%d x (%d x %d over %d x %d): the two gradient pairs do not leave as one chained launch", B, N_up, K_up, K_up, K_lo);
    GemmParams g[4];
    chain_shapes(B, N_up, K_up, K_lo, pu, pl, g);
    if (!afr_gemm_chain_block(g, block, member, tm, tn, slice)) return fail(AFR_EINVAL, "block %d: outside the chained launch", block);
    *phase = *member >= 2 ? 1 : 0;
    return AFR_OK;
}
// (l1: the first-layer role of afr_op_linear_chain_l1, its counters and target filled in here)
static int op_linear_chain(const void* dy, const void* x_up, const void* W_up, void* out_up, void* mid, const afr_linear_tail* tail_up,
                           const void* x_lo, const void* W_lo, void* out_lo, void* dx_lo, const afr_linear_tail* tail_lo,
                           int B, int N_up, int K_up, int K_lo, void* workspace, size_t workspace_bytes,
                           char* kernel_name, int name_cap, void* stream, ChainL1* l1) {
    static const afr_linear_tail none = {};
    const afr_linear_tail &tu = tail_up ? *tail_up : none, &tl = tail_lo ? *tail_lo : none;
    if (!dy || !x_up || !W_up || !out_up || !mid || !x_lo || !W_lo || !out_lo || !dx_lo) return fail(AFR_EINVAL, "null operand");
    if (kernel_name && name_cap < 1) return fail(AFR_EINVAL, "name_cap must be positive");
    if (B <= 0 || N_up <= 0 || K_up <= 0 || K_lo <= 0) return fail(AFR_EINVAL, "bad Linear extents");
    if (N_up % 8 || K_up % 8 || K_lo % 8) return fail(AFR_EUNSUPPORTED, "N and K must be multiples of 8");
    for (const afr_linear_tail* t : {&tu, &tl}) {
        if (t->target || t->target_rows || t->mask_out) return fail(AFR_EINVAL, "the fused loss and mask_out belong to AFR_LIN_FWD");
        const int K = t == &tu ? K_up : K_lo;
        if ((t->ld_out && t->ld_out != K) || (t->ldx && t->ldx != K && !t->x_rows) || (t->ldx && t->ldx < K)) return fail(AFR_EUNSUPPORTED, "afr_op_linear_chain: dense outputs and operands only");
        if (t->ld_db && t->ld_db < (t == &tu ? N_up : K_up)) return fail(AFR_EINVAL, "ld_db is smaller than its row");
    }
    size_t need = 0;
    int rc;
    if ((rc = afr_op_linear_chain_plan(B, N_up, K_up, K_lo, 0, nullptr, nullptr, nullptr, &need))) return rc;
    const size_t hb = align_up(((size_t)B + 255) / 256 * sizeof(unsigned), 256);
    if (l1) need += hb;
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 255)) return fail(AFR_EINVAL, "workspace missing, too small or misaligned: %zu < %zu", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    DevGuard dg(device_of(out_up));
    GemmParams g[4];
    PairPlan pu, pl;
    const size_t wu = pair_workspace_bytes(N_up, K_up, pair_plan_shape(B, N_up, K_up)), wl = pair_workspace_bytes(K_up, K_lo, pair_plan_shape(B, K_up, K_lo));
    char* w = (char*)workspace;
    if ((rc = linear_pair_members(AFR_BF16, tu, x_up, W_up, dy, out_up, mid, B, N_up, K_up, K_up, tu.ldx ? tu.ldx : K_up, tu.ld_db ? tu.ld_db : N_up, w, wu, s, g, &pu))) return rc;
    if ((rc = linear_pair_members(AFR_BF16, tl, x_lo, W_lo, mid, out_lo, dx_lo, B, K_up, K_lo, K_lo, tl.ldx ? tl.ldx : K_lo, tl.ld_db ? tl.ld_db : K_up, w + wu, wl, s, g + 2, &pl))) return rc;
    unsigned* hand = (unsigned*)(w + wu + wl);
    HIPCHK(hipMemsetAsync(hand, 0, l1 ? 2 * hb : hb, s));
    static uint32_t* err_word[16];       // a device word for AFR_ERR_COOP_TIMEOUT (no plan here): allocated once per device, never read back
    int dev = 0;
    uint32_t* err = nullptr;
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 16) {
        if (!err_word[dev]) { HIPCHK(hipMalloc((void**)&err_word[dev], 256)); HIPCHK(hipMemset(err_word[dev], 0, 256)); }
        err = err_word[dev];
    }
    g[0].err = err; g[2].err = err;
    if (l1) {
        l1->cnt = hand + hb / sizeof(unsigned); l1->target = afr_gemm_chain_l1_arrivals(g);
        if (!afr_gemm_chain_l1_ok(AFR_BF16, g, *l1))
            return fail(AFR_EUNSUPPORTED, "afr_op_linear_chain_l1: the first-layer backward does not ride this chained launch (d1 must be dx_lo, dense)");
    }
    if ((rc = launcher_rc(afr_launch_gemm_chain(AFR_BF16, g, hand, afr_gemm_chain_arrivals(g), err, s, l1), "chain"))) return rc;
    if (kernel_name) snprintf(kernel_name, name_cap, "%s", (tu.p && tu.opt_kind == AFR_OPT_LION) ? "gemm_bf16_group256_lion" : "gemm_bf16_group256");
    return AFR_OK;
}
extern "C" int afr_op_linear_chain(const void* dy, const void* x_up, const void* W_up, void* out_up, void* mid, const afr_linear_tail* tail_up,
                                   const void* x_lo, const void* W_lo, void* out_lo, void* dx_lo, const afr_linear_tail* tail_lo,
                                   int B, int N_up, int K_up, int K_lo, void* workspace, size_t workspace_bytes,
                                   char* kernel_name, int name_cap, void* stream) {
    return op_linear_chain(dy, x_up, W_up, out_up, mid, tail_up, x_lo, W_lo, out_lo, dx_lo, tail_lo, B, N_up, K_up, K_lo, workspace, workspace_bytes,
                           kernel_name, name_cap, stream, nullptr);
}
// ---- afr_op_linear_chain_l1: that launch with the folded first layer's fused backward as its fifth role (GemmGroup::l1), as a glyph
// step issues it: the refusals of afr_op_linear_chain and of afr_op_glyph_l1_bwd_fused (N1 = K_lo), and d1 must be dx_lo
static int glyph_op_shape(const char* what, int act_dtype, int B, int E, int vocab, int n_fonts);
static int glyph_op_n1(const char* what, int N1);
static int chain_l1_refusals(const char* what, int B, int N1, int vocab, int n_fonts, int ldh, bool rowmap) {
    if (int rc = glyph_op_shape(what, AFR_BF16, B, 32, vocab, n_fonts)) return rc;
    if (int rc = glyph_op_n1(what, N1)) return rc;
    if (!afr_glyph_l1_bwd_fused_eligible(AFR_BF16, 32, N1, vocab, n_fonts))
        return fail(AFR_EUNSUPPORTED, "%s: N1 = %d, vocab + n_fonts = %d: the fused backward takes N1 a multiple of 128 in 256 .. 1024 and at most 144 table rows (E = 32)",
                    what, N1, vocab + n_fonts);
    if (ldh < 32 || ldh % 8) return fail(AFR_EINVAL, "%s: ldh = %d must be a multiple of 8, at least 32", what, ldh);
    if ((long long)B * N1 * 2 >= (1ll << 31) || (!rowmap && (long long)B * ldh * 2 >= (1ll << 31)))
        return fail(AFR_EUNSUPPORTED, "%s: d1 and h0 must stay below 2 GiB", what);
    return AFR_OK;
}
extern "C" int afr_op_linear_chain_l1_plan(int B, int N_up, int K_up, int K_lo, int vocab, int n_fonts, int has_loss, int cus, int* blocks, size_t* workspace_bytes) {
    const char* what = "afr_op_linear_chain_l1";
    int nb = 0, rc;
    size_t ws = 0;
    if ((rc = afr_op_linear_chain_plan(B, N_up, K_up, K_lo, cus, nullptr, nullptr, &nb, &ws))) return rc;
    if ((rc = chain_l1_refusals(what, B, K_lo, vocab, n_fonts, 32, true))) return rc;
    if (blocks) *blocks = nb + afr_glyph_l1_bwd_fused_blocks(B, K_lo) + (has_loss ? 1 : 0);
    if (workspace_bytes) *workspace_bytes = ws + align_up(((size_t)B + 255) / 256 * sizeof(unsigned), 256);
    return AFR_OK;
}
extern "C" int afr_op_linear_chain_l1_block(int B, int N_up, int K_up, int K_lo, int vocab, int n_fonts, int has_loss, int block, int* role,
                                            int* row_block, int* col_range, int* wait_block) {
    if (!role || !row_block || !col_range || !wait_block) return fail(AFR_EINVAL, "null output");
    int nb = 0, rc;
    if ((rc = afr_op_linear_chain_l1_plan(B, N_up, K_up, K_lo, vocab, n_fonts, has_loss, 1 << 30, nullptr, nullptr))) return rc;
    if ((rc = afr_op_linear_chain_plan(B, N_up, K_up, K_lo, 1 << 30, nullptr, nullptr, &nb, nullptr))) return rc;
    *role = 0; *row_block = *col_range = *wait_block = -1;
    if (block >= 0 && block < nb) return AFR_OK;                   // a GEMM member: afr_op_linear_chain_block has its tile
    int ls = 0;
    if (!afr_gemm_chain_l1_block(B, K_lo, has_loss != 0, block - nb, row_block, col_range, wait_block, &ls))
        return fail(AFR_EINVAL, "block %d: outside the chained launch", block);
    *role = ls ? 2 : 1;
    return AFR_OK;
}
extern "C" int afr_op_linear_chain_l1(const void* dy, const void* x_up, const void* W_up, void* out_up, void* mid, const afr_linear_tail* tail_up,
                                      const void* x_lo, const void* W_lo, void* out_lo, void* dx_lo, const afr_linear_tail* tail_lo,
                                      int B, int N_up, int K_up, int K_lo, void* workspace, size_t workspace_bytes,
                                      const void* d1, const void* h0, int ldh, const int32_t* h0_rowmap, const void* W1T, const int64_t* x,
                                      const int64_t* font, int vocab, int n_fonts, float* slabs,
                                      const float* loss_partial, int loss_n, int loss_bd, float loss_inv_n, float* loss_accum,
                                      char* kernel_name, int name_cap, void* stream) {
    const char* what = "afr_op_linear_chain_l1";
    if (int rc = chain_l1_refusals(what, B, K_lo, vocab, n_fonts, ldh, h0_rowmap != nullptr)) return rc;
    if (!d1 || !h0 || !W1T || !x || !slabs) return fail(AFR_EINVAL, "%s: null argument", what);
    if (((uintptr_t)d1 & 15) || ((uintptr_t)h0 & 15) || ((uintptr_t)W1T & 15) || ((uintptr_t)slabs & 15))
        return fail(AFR_EINVAL, "%s: d1, h0, W1T and slabs must be 16-byte aligned", what);
    if (d1 != dx_lo) return fail(AFR_EUNSUPPORTED, "%s: d1 must be dx_lo, the lower input gradient this launch writes", what);
    if (loss_partial && (loss_n < 1 || (loss_bd != 256 && loss_bd != 512) || !loss_accum))
        return fail(AFR_EINVAL, "%s: deferred loss partials need n >= 1, a producer block size of 256 or 512 and an accumulator", what);
    ChainL1 l1;
    LossSum ls;
    l1.d1 = d1; l1.ldd = K_lo; l1.h0 = h0; l1.ldh = ldh; l1.h0_rowmap = h0_rowmap; l1.W1T = W1T; l1.x = x; l1.font = font;
    l1.B = B; l1.N1 = K_lo; l1.vocab = vocab; l1.n_fonts = n_fonts; l1.slabs = slabs;
    if (loss_partial) { ls.partial = loss_partial; ls.n = loss_n; ls.bd = loss_bd; ls.inv_n = loss_inv_n; ls.loss_accum = loss_accum; l1.loss = &ls; }
    return op_linear_chain(dy, x_up, W_up, out_up, mid, tail_up, x_lo, W_lo, out_lo, dx_lo, tail_lo, B, N_up, K_up, K_lo, workspace, workspace_bytes,
                           kernel_name, name_cap, stream, &l1);
}
extern "C" int afr_op_reduce(float* dst, const float* slabs, int nslabs, int64_t stride, int64_t n, float scale, int acc,
                             void* stream) {
    if (!dst || !slabs || nslabs < 1) return fail(AFR_EINVAL, "bad reduce arguments");
    DevGuard dg(device_of(dst));
    HIPCHK(afr_launch_reduce(dst, slabs, nslabs, stride, n, scale, acc, (hipStream_t)stream));
    return AFR_OK;
}
// ---- afr_op_reduce_group_step: the grouped reduce as reduce_and_step issues it (afr_rtable_add, adam_hyper, group_args, the launcher)
extern "C" int afr_op_reduce_group_step(int nseg, float* const* dst, const float* const* slabs, const int* nslabs, const int64_t* stride,
                                        const int64_t* n, const afr_reduce_step* step, char* kernel_name, int name_cap, void* stream) {
    const char* who = "afr_op_reduce_group_step";
    if (nseg < 1 || nseg > AFR_RT_MAXSEG) return fail(AFR_EINVAL, "a grouped reduce takes 1 to at most %d segments (got %d)", AFR_RT_MAXSEG, nseg);
    if (!dst || !slabs || !nslabs || !stride || !n) return fail(AFR_EINVAL, "%s: null segment array", who);
    if (kernel_name && name_cap < 1) return fail(AFR_EINVAL, "%s: name_cap must be positive", who);
    const bool fused = step && step->p;
    const int kind = fused ? step->opt_kind : OPT_ADAMW;
    if (step && !fused && step->shT) {
        for (int i = 0; i < nseg; ++i) if (step->shT[i]) return fail(AFR_EINVAL, "segment %d: shT without a fused step (step->p is null)", i);
    }
    AdamArgs h{};
    if (fused) {
        if (kind != AFR_OPT_ADAMW && kind != AFR_OPT_LION) return fail(AFR_EINVAL, "optimizer kind must be AFR_OPT_ADAMW (0) or AFR_OPT_LION (1), got %d", kind);
        if (!step->gbase || !step->m || (kind == AFR_OPT_ADAMW && !step->v)) return fail(AFR_EINVAL, "%s: fused step: null gbase or moment", who);
        if (step->shT && (!step->tN || !step->tK)) return fail(AFR_EINVAL, "%s: shT without tN and tK", who);
        if (kind == AFR_OPT_ADAMW) if (int rc = check_step_count(step->t)) return rc;
        h = AdamArgs{step->lr, step->beta1, step->beta2, step->eps, step->weight_decay, kind == AFR_OPT_LION ? 1 : step->t};
    }
    const bool grouped = fused && (step->lr_mult || step->wd_mult);
    RTable rt;
    AdamHyper seg_ad[AFR_RT_MAXSEG];
    if (fused) {
        rt.adam = 1; rt.ad = adam_hyper(h, kind); rt.kind = kind;
        rt.gbase = step->gbase; rt.P = step->p; rt.M = step->m; rt.V = kind == OPT_LION ? nullptr : step->v; rt.shadow = (bf16_t*)step->shadow;
    }
    for (int i = 0; i < nseg; ++i) {
        if (!dst[i] || !slabs[i]) return fail(AFR_EINVAL, "segment %d: null pointer", i);
        if (nslabs[i] < 1) return fail(AFR_EINVAL, "segment %d: nslabs = %d, must be >= 1", i, nslabs[i]);
        if (n[i] < 0 || (n[i] & 3)) return fail(AFR_EINVAL, "segment %d: length %lld is negative or not a multiple of 4", i, (long long)n[i]);
        if (stride[i] & 3) return fail(AFR_EINVAL, "segment %d: stride %lld is not a multiple of 4", i, (long long)stride[i]);
        afr_opt_range r{0, 1.f, 1.f};
        if (fused) {
            const ptrdiff_t off = (const char*)dst[i] - (const char*)step->gbase;
            if (off < 0 || (off & 15)) return fail(AFR_EINVAL, "segment %d: dst - gbase is negative or not a multiple of 4 elements", i);
            if (step->lr_mult) r.lr_mult = step->lr_mult[i];
            if (step->wd_mult) r.wd_mult = step->wd_mult[i];
            if (!mult_ok(r.lr_mult) || !mult_ok(r.wd_mult)) return fail(AFR_EINVAL, "segment %d: the multipliers must be finite and >= 0", i);
            if (step->shT && step->shT[i]) {
                const int tN = step->tN[i], tK = step->tK[i];
                if (tK < 4 || tK % 4) return fail(AFR_EINVAL, "segment %d: shT with tK = %d, must be a positive multiple of 4", i, tK);
                if (n[i] % tK) return fail(AFR_EINVAL, "segment %d: shT with a length %lld that is no multiple of tK = %d", i, (long long)n[i], tK);
                if (tN < n[i] / tK) return fail(AFR_EINVAL, "segment %d: shT with pitch tN = %d smaller than its %lld rows", i, tN, (long long)(n[i] / tK));
            }
        }
        const int k = rt.nseg;            // the table's number of this segment: afr_rtable_add drops a segment with n == 0
        afr_rtable_add(rt, dst[i], slabs[i], nslabs[i], stride[i], n[i]);
        if (rt.nseg == k || !fused) continue;
        seg_ad[k] = adam_hyper(group_args(h, r), kind);
        if (step->shT && step->shT[i]) { rt.seg[k].shT = (bf16_t*)step->shT[i]; rt.seg[k].tN = step->tN[i]; rt.seg[k].tK = step->tK[i]; }
    }
    if (kernel_name) snprintf(kernel_name, name_cap, "%s", afr_reduce_group_kernel_name(rt, grouped ? seg_ad : nullptr));
    DevGuard dg(device_of(fused ? (const void*)step->p : (const void*)dst[0]));
    HIPCHK(afr_launch_reduce_group(rt, (hipStream_t)stream, grouped ? seg_ad : nullptr));
    return AFR_OK;
}
// (no segments: nothing to do, as it has always answered; everything else is the step form's, refusals included)
extern "C" int afr_op_reduce_group(int nseg, float* const* dst, const float* const* slabs, const int* nslabs, const int64_t* stride,
                                   const int64_t* n, void* stream) {
    if (nseg == 0) return AFR_OK;
    return afr_op_reduce_group_step(nseg, dst, slabs, nslabs, stride, n, nullptr, nullptr, 0, stream);
}
extern "C" int afr_op_adamw(float* p, const float* g, float* m, float* v, void* shadow, int64_t n, float lr, float b1,
                            float b2, float eps, float wd, int64_t t, float gscale, void* stream) {
    if (!p || !g || !m || !v || t < 1) return fail(AFR_EINVAL, "bad AdamW arguments");
    DevGuard dg(device_of(p));
    return flat_step(OPT_ADAMW, p, g, m, v, (bf16_t*)shadow, n, AdamArgs{lr, b1, b2, eps, wd, t}, gscale, (hipStream_t)stream);
}
extern "C" int afr_op_adamw_clip(float* p, const float* g, float* m, float* v, void* shadow, int64_t n, float lr, float b1, float b2,
                                 float eps, float wd, int64_t t, float gscale, const float* sumsq, float max_norm, void* stream) {
    if (!p || !g || !m || !v || !sumsq) return fail(AFR_EINVAL, "null argument");
    if (int rc = check_step_count(t)) return rc;
    if (!(max_norm > 0.f) || std::isinf(max_norm)) return fail(AFR_EINVAL, "max_norm must be finite and > 0, got %g", (double)max_norm);
    DevGuard dg(device_of(p));
    return flat_step(OPT_ADAMW, p, g, m, v, (bf16_t*)shadow, n, AdamArgs{lr, b1, b2, eps, wd, t}, gscale, (hipStream_t)stream, sumsq, max_norm);
}
extern "C" int afr_op_lion(float* p, const float* g, float* m, void* shadow, int64_t n, float lr, float b1, float b2, float wd,
                           float gscale, const float* sumsq, float max_norm, void* stream) {
    if (!p || !g || !m) return fail(AFR_EINVAL, "null argument");
    if (sumsq && (!(max_norm > 0.f) || std::isinf(max_norm))) return fail(AFR_EINVAL, "max_norm must be finite and > 0, got %g", (double)max_norm);
    DevGuard dg(device_of(p));
    return flat_step(OPT_LION, p, g, m, nullptr, (bf16_t*)shadow, n, AdamArgs{lr, b1, b2, 0.f, wd, 1}, gscale, (hipStream_t)stream, sumsq, max_norm);
}
extern "C" int afr_op_opt_groups(int kind, float* p, const float* g, float* m, float* v, void* shadow, int64_t n, int64_t first,
                                 const afr_opt_range* ranges, int n_ranges, float lr, float b1, float b2, float eps, float wd, int64_t t, float gscale,
                                 const float* sumsq, float max_norm, void* stream) {
    if (kind != AFR_OPT_ADAMW && kind != AFR_OPT_LION) return fail(AFR_EINVAL, "optimizer kind must be AFR_OPT_ADAMW (0) or AFR_OPT_LION (1), got %d", kind);
    if (!p || !g || !m || (kind == AFR_OPT_ADAMW && !v)) return fail(AFR_EINVAL, "null argument");
    if (int rc = check_step_count(t)) return rc;
    if (sumsq && (!(max_norm > 0.f) || std::isinf(max_norm))) return fail(AFR_EINVAL, "max_norm must be finite and > 0, got %g", (double)max_norm);
    DevGuard dg(device_of(p));
    const FlatRanges rg{ranges, n_ranges, first};
    return flat_step(kind, p, g, m, v, (bf16_t*)shadow, n, AdamArgs{lr, b1, b2, eps, wd, kind == AFR_OPT_LION ? 1 : t}, gscale, (hipStream_t)stream, sumsq, max_norm,
                     &rg);
}
extern "C" int afr_op_mse_grad(int act_dtype, const void* u, const void* target, int tdtype, void* du, int64_t rows,
                               int64_t cols, int64_t mean_elems, float* loss_accum, float* scratch, void* stream) {
    if (!u || !target || !du || !loss_accum || !scratch) return fail(AFR_EINVAL, "null argument");
    DevGuard dg(device_of(du));
    HIPCHK(afr_launch_mse_grad(act_dtype, u, du, rows, cols, loss_args(scratch, false, AFR_LOSS_MSE, target, tdtype, nullptr, mean_elems, loss_accum), (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_bce_grad(int act_dtype, const void* u, const void* target, int tdtype, void* du, int64_t rows,
                               int64_t cols, int64_t mean_elems, float* loss_accum, float* scratch, void* stream) {
    if (!u || !target || !du || !loss_accum || !scratch) return fail(AFR_EINVAL, "null argument");
    DevGuard dg(device_of(du));
    HIPCHK(afr_launch_mse_grad(act_dtype, u, du, rows, cols, loss_args(scratch, false, AFR_LOSS_BCE, target, tdtype, nullptr, mean_elems, loss_accum), (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_eval(int act_dtype, int loss_kind, const void* u, const void* target, int tdtype, const int32_t* rowmap, int64_t rows,
                           int64_t cols, float* loss_rows, uint32_t* stats, uint8_t* q, void* stream) {
    if (!u) return fail(AFR_EINVAL, "afr_op_eval: u is null");
    if (act_dtype != AFR_F32 && act_dtype != AFR_BF16) return fail(AFR_EINVAL, "afr_op_eval: act_dtype must be AFR_F32 or AFR_BF16");
    if (loss_kind != AFR_LOSS_MSE && loss_kind != AFR_LOSS_BCE) return fail(AFR_EINVAL, "afr_op_eval: loss_kind must be AFR_LOSS_MSE (0) or AFR_LOSS_BCE (1), got %d", loss_kind);
    if (!loss_rows && !stats && !q) return fail(AFR_EINVAL, "afr_op_eval: loss_rows, stats and q are all NULL");
    if (!target && (loss_rows || stats)) return fail(AFR_EINVAL, "afr_op_eval: loss_rows and stats need a target");
    if (target && tdtype != AFR_TARGET_U8 && tdtype != AFR_TARGET_F32) return fail(AFR_EINVAL, "bad target dtype");
    if (rows <= 0 || cols <= 0) return fail(AFR_EINVAL, "afr_op_eval: rows and cols must be positive");
    if (cols % 8) return fail(AFR_EUNSUPPORTED, "afr_op_eval: cols must be a multiple of 8 (got %lld)", (long long)cols);
    if (((uintptr_t)u & 15) || ((uintptr_t)stats & 15) || ((uintptr_t)q & 7) || ((uintptr_t)loss_rows & 3) || ((uintptr_t)rowmap & 3) ||
        ((uintptr_t)target & (tdtype == AFR_TARGET_U8 ? 7 : 15)))
        return fail(AFR_EINVAL, "afr_op_eval: u, stats and float32 targets must be 16-byte aligned, q and uint8 targets 8-byte");
    DevGuard dg(device_of(u));
    HIPCHK(afr_launch_eval_rows(act_dtype, loss_kind, u, target, tdtype, target ? rowmap : nullptr, rows, cols, loss_rows, stats, q, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream) {
    DevGuard dg(device_of(dst));
    HIPCHK(afr_launch_f32_to_bf16(src, (bf16_t*)dst, n, (hipStream_t)stream));
    return AFR_OK;
}
// What the three afr_op_dataset_text* entries refuse alike: `table` is the entry's letter table under its name (cum / cum2), both null for
// the entry without one, which then has no err word either.  -> AFR_OK or the failure, already recorded.
static int text_args_check(const char* who, const int64_t* seed_rows, const int64_t* out_rows, int64_t n, int min_len, int max_len,
                           const char* table_name, const uint32_t* table, const int64_t* codes, int ldx, const int32_t* len, const uint32_t* err) {
    if (!codes || (table_name && !table))
        return table_name ? fail(AFR_EINVAL, "%s: codes or %s is null", who, table_name) : fail(AFR_EINVAL, "%s: codes is null", who);
    if (n < 1) return fail(AFR_EINVAL, "%s: n = %lld, must be >= 1", who, (long long)n);
    if (ldx < 1) return fail(AFR_EINVAL, "%s: ldx = %d, must be positive", who, ldx);
    if (ldx > CMP_MAX_LDX) return fail(AFR_EUNSUPPORTED, "%s: ldx = %d, at most %d codes per row", who, ldx, CMP_MAX_LDX);
    if (min_len < 1 || max_len < min_len || max_len > ldx)
        return fail(AFR_EINVAL, "%s: text lengths %d..%d must satisfy 1 <= min_len <= max_len <= ldx = %d", who, min_len, max_len, ldx);
    if (((uintptr_t)codes & 7) || ((uintptr_t)seed_rows & 7) || ((uintptr_t)out_rows & 7) || ((uintptr_t)len & 3) || ((uintptr_t)table & 3) ||
        ((uintptr_t)err & 3))
        return table_name ? fail(AFR_EINVAL, "%s: codes, seed_rows and out_rows must be 8-byte aligned, %s, len and err 4-byte", who, table_name)
                          : fail(AFR_EINVAL, "%s: codes, seed_rows and out_rows must be 8-byte aligned, len 4-byte", who);
    return AFR_OK;
}
extern "C" int afr_op_dataset_text(int64_t first_seed, const int64_t* seed_rows, const int64_t* out_rows, int64_t n, int min_len, int max_len,
                                   int64_t* codes, int ldx, int32_t* len, void* stream) {
    if (const int rc = text_args_check("afr_op_dataset_text", seed_rows, out_rows, n, min_len, max_len, nullptr, nullptr, codes, ldx, len, nullptr))
        return rc;
    DevGuard dg(device_of(codes));
    HIPCHK(afr_launch_dataset_text(first_seed, seed_rows, out_rows, n, min_len, max_len, codes, ldx, len, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_dataset_text_w(int64_t first_seed, const int64_t* seed_rows, const int64_t* out_rows, int64_t n, int min_len, int max_len,
                                     const uint32_t* cum, int64_t* codes, int ldx, int32_t* len, uint32_t* err, void* stream) {
    if (const int rc = text_args_check("afr_op_dataset_text_w", seed_rows, out_rows, n, min_len, max_len, "cum", cum, codes, ldx, len, err)) return rc;
    DevGuard dg(device_of(codes));
    HIPCHK(afr_launch_dataset_text_w(first_seed, seed_rows, out_rows, n, min_len, max_len, cum, codes, ldx, len, err, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_dataset_text_m(int64_t first_seed, const int64_t* seed_rows, const int64_t* out_rows, int64_t n, int min_len, int max_len,
                                     const uint32_t* cum2, int64_t* codes, int ldx, int32_t* len, uint32_t* err, void* stream) {
    if (const int rc = text_args_check("afr_op_dataset_text_m", seed_rows, out_rows, n, min_len, max_len, "cum2", cum2, codes, ldx, len, err)) return rc;
    DevGuard dg(device_of(codes));
    HIPCHK(afr_launch_dataset_text_m(first_seed, seed_rows, out_rows, n, min_len, max_len, cum2, codes, ldx, len, err, (hipStream_t)stream));
    return AFR_OK;
}
// What afr_op_text_weights and afr_op_pair_weights refuse alike: the member mask, the weight ranges and the alignment of the counter table
// and of the two outputs, each under its name; n_codes is how many codes a given table holds (the pair table's shape is fixed: it holds
// them all).  -> AFR_OK or the failure, already recorded.
static int weights_args_check(const char* who, const char* table_name, const uint64_t* table, int n_codes, const uint32_t* members,
                              uint32_t floor_w, uint32_t gain, const char* cum_name, const uint32_t* cum, const char* w_name, const uint32_t* w) {
    if (!members || !cum) return fail(AFR_EINVAL, "%s: members or %s is null", who, cum_name);
    if (table && n_codes < AFR_TEXT_FIRST + AFR_TEXT_CODES)
        return fail(AFR_EINVAL, "%s: n_codes = %d, a by-code table must hold the codes up to %d", who, n_codes, AFR_TEXT_FIRST + AFR_TEXT_CODES - 1);
    if (members[2] >> (AFR_TEXT_CODES - 64))
        return fail(AFR_EINVAL, "%s: member bits above bit %d (code %d) are set", who, AFR_TEXT_CODES - 1, AFR_TEXT_FIRST + AFR_TEXT_CODES - 1);
    if (!(members[0] | members[1] | members[2])) return fail(AFR_EINVAL, "%s: the member set is empty", who);
    if (floor_w < 1u || floor_w > 65535u || gain > 65535u)
        return fail(AFR_EINVAL, "%s: floor_w = %u must lie in 1..65535, gain = %u in 0..65535", who, floor_w, gain);
    if (((uintptr_t)table & 7) || ((uintptr_t)cum & 3) || ((uintptr_t)w & 3))
        return fail(AFR_EINVAL, "%s: %s must be 8-byte aligned, %s and %s 4-byte", who, table_name, cum_name, w_name);
    return AFR_OK;
}
extern "C" int afr_op_text_weights(const uint64_t* by_code, int n_codes, const uint32_t* members, uint32_t floor_w, uint32_t gain, uint32_t* cum,
                                   uint32_t* w, void* stream) {
    if (const int rc = weights_args_check("afr_op_text_weights", "by_code", by_code, n_codes, members, floor_w, gain, "cum", cum, "w", w)) return rc;
    DevGuard dg(device_of(cum));
    HIPCHK(afr_launch_text_weights((const unsigned long long*)by_code, members, floor_w, gain, cum, w, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_pair_errors(const int64_t* codes, int ldx, const int64_t* code_rows, int64_t n, const uint32_t* per_pos, uint64_t* by_pair,
                                  void* stream) {
    const char* who = "afr_op_pair_errors";
    if (!codes || !per_pos || !by_pair) return fail(AFR_EINVAL, "%s: codes, per_pos or by_pair is null", who);
    if (n < 1) return fail(AFR_EINVAL, "%s: n = %lld, must be >= 1", who, (long long)n);
    if (ldx < 1) return fail(AFR_EINVAL, "%s: ldx = %d, must be positive", who, ldx);
    if (ldx > CMP_MAX_LDX) return fail(AFR_EUNSUPPORTED, "%s: ldx = %d, at most %d codes per row", who, ldx, CMP_MAX_LDX);
    if (((uintptr_t)codes & 7) || ((uintptr_t)code_rows & 7) || ((uintptr_t)by_pair & 7) || ((uintptr_t)per_pos & 15))
        return fail(AFR_EINVAL, "%s: codes, code_rows and by_pair must be 8-byte aligned, per_pos 16-byte", who);
    DevGuard dg(device_of(by_pair));
    HIPCHK(afr_launch_pair_errors(codes, ldx, code_rows, n, per_pos, (unsigned long long*)by_pair, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_pair_weights(const uint64_t* by_pair, const uint32_t* members, uint32_t floor_w, uint32_t gain, uint32_t min_chars,
                                   uint32_t* cum2, uint32_t* w2, void* stream) {
    if (const int rc = weights_args_check("afr_op_pair_weights", "by_pair", by_pair, AFR_TEXT_FIRST + AFR_TEXT_CODES, members, floor_w, gain, "cum2", cum2, "w2", w2)) return rc;
    DevGuard dg(device_of(cum2));
    HIPCHK(afr_launch_pair_weights((const unsigned long long*)by_pair, members, floor_w, gain, min_chars, cum2, w2, (hipStream_t)stream));
    return AFR_OK;
}
// What afr_op_compose_sheets, afr_op_sheet_char_errors and afr_op_sheet_read_back refuse alike: `dense` is the sheet-shaped buffer
// (out / pred), `rows` the row vector, lds_extra which kernel's LDS need is held against the budget.  -> AFR_OK or the failure, already recorded.
enum { SHEET_LDS_COMPOSE = 0, SHEET_LDS_CHARERR = 1, SHEET_LDS_READBACK = 2 };
static int sheet_args_check(const char* who, const char* dense_name, const afr_glyph_atlas* atlas, const afr_sheet_geometry* geo,
                            const int64_t* codes, int ldx, const int64_t* rows, int64_t n, const void* dense, const uint32_t* err,
                            int lds_extra) {
    if (!atlas || !geo || !codes || !dense) return fail(AFR_EINVAL, "%s: atlas, geo, codes or %s is null", who, dense_name);
    if (!atlas->cells || !atlas->adv64) return fail(AFR_EINVAL, "%s: the atlas's cells or adv64 is null", who);
    if (n < 1) return fail(AFR_EINVAL, "%s: n = %lld, must be >= 1", who, (long long)n);
    if (geo->n_lines < 1 || geo->n_lines > CMP_MAX_LINES)
        return fail(AFR_EINVAL, "%s: n_lines = %d, must be 1..%d", who, geo->n_lines, CMP_MAX_LINES);
    if (atlas->n_codes < 1 || atlas->cell_h < 1 || atlas->cell_w < 1 || geo->height < 1 || geo->width < 1 || ldx < 1 || geo->wrap_width64 < 0)
        return fail(AFR_EINVAL, "%s: sizes must be positive (n_codes %d, cell %d x %d, sheet %d x %d, ldx %d, wrap_width64 %d)", who,
                    atlas->n_codes, atlas->cell_h, atlas->cell_w, geo->height, geo->width, ldx, geo->wrap_width64);
    if (atlas->origin_x < 0 || atlas->origin_x >= atlas->cell_w || atlas->origin_y < 0 || atlas->origin_y >= atlas->cell_h)
        return fail(AFR_EINVAL, "%s: origin (%d, %d) outside the %d x %d cell", who, atlas->origin_x, atlas->origin_y, atlas->cell_w,
                    atlas->cell_h);
    if (((uintptr_t)atlas->cells & 3) || ((uintptr_t)atlas->adv64 & 3) || ((uintptr_t)atlas->kern64 & 1) || ((uintptr_t)codes & 7) ||
        ((uintptr_t)rows & 7) || ((uintptr_t)dense & 7) || ((uintptr_t)err & 3))
        return fail(AFR_EINVAL, "%s: %s, codes and the row vector must be 8-byte aligned, cells, adv64 and err 4-byte, kern64 2-byte", who, dense_name);
    if (ldx > CMP_MAX_LDX) return fail(AFR_EUNSUPPORTED, "%s: ldx = %d, at most %d codes per row", who, ldx, CMP_MAX_LDX);
    if (geo->width % 8) return fail(AFR_EUNSUPPORTED, "%s: width must be a multiple of 8 (got %d)", who, geo->width);
    if ((long long)geo->height * geo->width >= (1ll << 31))
        return fail(AFR_EUNSUPPORTED, "%s: a sheet of %d x %d pixels is 2 GiB or more", who, geo->height, geo->width);
    if ((long long)atlas->n_codes * atlas->cell_h * atlas->cell_w > AFR_COMPOSE_LDS_BUDGET || geo->width / 8 > AFR_COMPOSE_LDS_BUDGET)
        return fail(AFR_EUNSUPPORTED, "%s: the atlas's cells (%d x %d x %d bytes) or a row of %d pixels alone pass the LDS budget of %d bytes", who,
                    atlas->n_codes, atlas->cell_h, atlas->cell_w, geo->width, AFR_COMPOSE_LDS_BUDGET);
    const int nc = atlas->n_codes, ch = atlas->cell_h, cw = atlas->cell_w;
    const long long lds = lds_extra == SHEET_LDS_READBACK ? (long long)afr_readback_dynamic_lds(nc, ch, cw, geo->n_lines, geo->width) + (long long)afr_readback_static_lds()
                          : lds_extra == SHEET_LDS_CHARERR ? (long long)afr_charerr_dynamic_lds(nc, ch, cw, geo->n_lines, geo->width) + (long long)afr_charerr_static_lds()
                                                           : (long long)afr_compose_dynamic_lds(nc, ch, cw, geo->n_lines, geo->width) + (long long)afr_compose_static_lds();
    if (lds > AFR_COMPOSE_LDS_BUDGET)
        return fail(AFR_EUNSUPPORTED, "%s: the atlas's cells (%d x %d x %d bytes), the glyph ranges and the layout%s need %lld bytes of LDS, the budget is %d",
                    who, nc, ch, cw,
                    lds_extra == SHEET_LDS_READBACK  ? ", the position records, the waves' windows and the confusion counters"
                    : lds_extra == SHEET_LDS_CHARERR ? ", the position records and the code counters"
                                                     : "",
                    lds, AFR_COMPOSE_LDS_BUDGET);
    return AFR_OK;
}
static ComposeArgs compose_args(const afr_glyph_atlas* atlas, const afr_sheet_geometry* geo, const int64_t* codes, int ldx, const int64_t* rows,
                                int64_t n, uint8_t* out, uint32_t* err) {
    ComposeArgs a{atlas->cells, atlas->adv64, atlas->kern64, atlas->n_codes, atlas->cell_h, atlas->cell_w, atlas->origin_x, atlas->origin_y,
                  geo->height, geo->width, geo->wrap_width64, geo->n_lines, {}, codes, ldx, rows, n, out, err};
    for (int i = 0; i < CMP_MAX_LINES; ++i) a.baseline[i] = i < geo->n_lines ? geo->baseline[i] : 0;
    return a;
}
extern "C" int afr_op_compose_sheets(const afr_glyph_atlas* atlas, const afr_sheet_geometry* geo, const int64_t* codes, int ldx,
                                     const int64_t* out_rows, int64_t n, uint8_t* out, uint32_t* err, void* stream) {
    if (const int rc = sheet_args_check("afr_op_compose_sheets", "out", atlas, geo, codes, ldx, out_rows, n, out, err, SHEET_LDS_COMPOSE)) return rc;
    const ComposeArgs a = compose_args(atlas, geo, codes, ldx, out_rows, n, out, err);
    DevGuard dg(device_of(out));
    HIPCHK(afr_launch_compose_sheets(a, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_sheet_char_errors(const afr_glyph_atlas* atlas, const afr_sheet_geometry* geo, const int64_t* codes, int ldx,
                                        const int64_t* code_rows, int64_t n, const uint8_t* pred, uint32_t* per_pos, uint64_t* by_code,
                                        uint32_t* err, void* stream) {
    const char* who = "afr_op_sheet_char_errors";
    if (const int rc = sheet_args_check(who, "pred", atlas, geo, codes, ldx, code_rows, n, pred, err, SHEET_LDS_CHARERR)) return rc;
    // a record's sumsq is a uint32: 255^2 * pixels must fit
    if ((long long)geo->height * geo->width > 66051)
        return fail(AFR_EUNSUPPORTED, "%s: a sheet of %d x %d pixels: 65025 * pixels must fit 32 bits, at most 66051 pixels", who, geo->height,
                    geo->width);
    if (!per_pos && !by_code) return fail(AFR_EINVAL, "%s: per_pos and by_code are both NULL", who);
    if (((uintptr_t)per_pos & 15) || ((uintptr_t)by_code & 7))
        return fail(AFR_EINVAL, "%s: per_pos must be 16-byte aligned, by_code 8-byte", who);
    const CharErrArgs a{compose_args(atlas, geo, codes, ldx, code_rows, n, nullptr, err), pred, per_pos, (unsigned long long*)by_code};
    DevGuard dg(device_of(pred));
    HIPCHK(afr_launch_sheet_char_errors(a, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_sheet_read_back(const afr_glyph_atlas* atlas, const afr_sheet_geometry* geo, const int64_t* codes, int ldx,
                                      const int64_t* code_rows, int64_t n, const uint8_t* pred, const uint32_t* members, uint8_t* read,
                                      uint32_t* score, uint64_t* confusion, uint32_t* err, void* stream) {
    const char* who = "afr_op_sheet_read_back";
    if (!atlas || !geo) return fail(AFR_EINVAL, "%s: atlas or geo is null", who);
    // a window's score is a uint32: 255^2 * pixels must fit (asked before the LDS budget, which such a cell passes as well)
    if ((long long)atlas->cell_h * atlas->cell_w > 66051)
        return fail(AFR_EUNSUPPORTED, "%s: a cell of %d x %d pixels: 65025 * pixels must fit 32 bits, at most 66051 pixels", who, atlas->cell_h,
                    atlas->cell_w);
    if (const int rc = sheet_args_check(who, "pred", atlas, geo, codes, ldx, code_rows, n, pred, err, SHEET_LDS_READBACK)) return rc;
    if (!members) return fail(AFR_EINVAL, "%s: members is null", who);
    if (members[2] >> (AFR_TEXT_CODES - 64))
        return fail(AFR_EINVAL, "%s: member bits above bit %d (code %d) are set", who, AFR_TEXT_CODES - 1, AFR_TEXT_FIRST + AFR_TEXT_CODES - 1);
    if (atlas->n_codes < AFR_TEXT_FIRST + AFR_TEXT_CODES)
        return fail(AFR_EINVAL, "%s: n_codes = %d, the atlas must hold the candidates' cells, the codes up to %d", who, atlas->n_codes,
                    AFR_TEXT_FIRST + AFR_TEXT_CODES - 1);
    if (atlas->n_codes > 256) return fail(AFR_EUNSUPPORTED, "%s: n_codes = %d, a code read back is stored in a byte: at most 256", who, atlas->n_codes);
    if (!read && !score && !confusion) return fail(AFR_EINVAL, "%s: read, score and confusion are all NULL", who);
    if (((uintptr_t)score & 7) || ((uintptr_t)confusion & 7)) return fail(AFR_EINVAL, "%s: score and confusion must be 8-byte aligned", who);
    const ReadBackArgs a{compose_args(atlas, geo, codes, ldx, code_rows, n, nullptr, err), pred, {members[0], members[1], members[2]}, read, score,
                         (unsigned long long*)confusion};
    DevGuard dg(device_of(pred));
    HIPCHK(afr_launch_sheet_read_back(a, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_f32_to_fp8(const float* src, void* dst, int64_t n, float scale, void* stream) {
    if (!src || !dst || n < 0 || !(scale > 0.f)) return fail(AFR_EINVAL, "bad f32 -> fp8 arguments");
    DevGuard dg(device_of(dst));
    HIPCHK(afr_launch_f32_to_fp8(src, (unsigned char*)dst, n, scale, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_gemm_fp8(int flags, const void* A, const void* B, void* C, const float* bias, int M, int N, int K, int lda, int ldb,
                               int ldc, float scale_ab, void* stream) {
    if (!A || !B || !C) return fail(AFR_EINVAL, "null operand");
    if (M <= 0 || N <= 0 || K <= 0) return fail(AFR_EINVAL, "bad GEMM extents");
    if (flags & ~(AFR_GEMM_BIAS | AFR_GEMM_RELU | AFR_GEMM_OUT_BF16)) return fail(AFR_EUNSUPPORTED, "fp8 products take bias / relu / bf16-output only (both operands k-contiguous)");
    if ((flags & AFR_GEMM_BIAS) && !bias) return fail(AFR_EINVAL, "bias flag without a bias");
    if (K % 16 || lda % 16 || ldb % 16 || N % 8 || ldc % 8) return fail(AFR_EUNSUPPORTED, "K, lda, ldb must be multiples of 16; N, ldc of 8");
    if ((long long)M * lda >= (1ll << 31) || (long long)N * ldb >= (1ll << 31)) return fail(AFR_EUNSUPPORTED, "an fp8 GEMM operand must be smaller than 2 GiB");
    DevGuard dg(device_of(C));
    GemmParams g;
    g.A = A; g.B = B; g.C = C; g.bias = bias; g.aux = nullptr; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldaux = 0;
    g.flags = flags; g.splitk = 1; g.slab_stride = 0; g.out_scale = scale_ab;
    HIPCHK(afr_launch_gemm_fp8(g, (hipStream_t)stream));
    return AFR_OK;
}

// ---- the pixel transformer's token kernels one launch each (include/afr.h): argument checks, then the launcher the plan calls
static int pixel_op_shape(const char* what, int act_dtype, long long rows, int d) {
    if (act_dtype != AFR_F32 && act_dtype != AFR_BF16) return fail(AFR_EINVAL, "%s: act_dtype must be AFR_F32 or AFR_BF16, got %d", what, act_dtype);
    if (rows < 1) return fail(AFR_EINVAL, "%s: rows = %lld must be >= 1", what, rows);
    if (d < 64 || d > 512 || d % 64) return fail(AFR_EUNSUPPORTED, "%s: d = %d must be 64 * heads <= 512", what, d);
    return AFR_OK;
}
static int pixel_op_attn_shape(const char* what, int tokens, int d, int heads, int C) {
    if (tokens < 1) return fail(AFR_EINVAL, "%s: tokens = %d must be >= 1", what, tokens);
    if (d != 64 * heads) return fail(AFR_EUNSUPPORTED, "%s: d = %d must be 64 * heads (heads = %d)", what, d, heads);
    if (C < 1 || C > 2) return fail(AFR_EINVAL, "%s: C = %d context tokens, must be 1 or 2", what, C);
    return AFR_OK;
}
extern "C" int afr_op_pixel_ctx(int act_dtype, const float* emb, const float* femb, const int64_t* x, const int64_t* font, int B, int d, int vocab,
                                int n_fonts, void* ctx, uint32_t* err, void* stream) {
    if (int rc = pixel_op_shape("afr_op_pixel_ctx", act_dtype, B, d)) return rc;
    if (!emb || !x || !ctx || !err || (n_fonts > 0 && (!femb || !font))) return fail(AFR_EINVAL, "afr_op_pixel_ctx: null argument");
    if (vocab < 1 || n_fonts < 0) return fail(AFR_EINVAL, "afr_op_pixel_ctx: vocab = %d, n_fonts = %d", vocab, n_fonts);
    DevGuard dg(device_of(ctx));
    HIPCHK(afr_launch_pixel_ctx(act_dtype, emb, femb, x, font, B, d, vocab, n_fonts, ctx, err, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_pixel_ctx_bwd(const float* dctx, const int64_t* x, const int64_t* font, int B, int d, int vocab, int n_fonts, float* demb,
                                    float* dfont, void* stream) {
    if (int rc = pixel_op_shape("afr_op_pixel_ctx_bwd", AFR_F32, B, d)) return rc;
    if (!dctx || !x || !demb || (n_fonts > 0 && (!font || !dfont))) return fail(AFR_EINVAL, "afr_op_pixel_ctx_bwd: null argument");
    if (vocab < 1 || n_fonts < 0) return fail(AFR_EINVAL, "afr_op_pixel_ctx_bwd: vocab = %d, n_fonts = %d", vocab, n_fonts);
    DevGuard dg(device_of(demb));
    HIPCHK(afr_launch_pixel_ctx_bwd(dctx, x, font, B, d, vocab, n_fonts, demb, dfont, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_pixel_add_ln(int act_dtype, const float* hin, float* h, const float* pos, const void* add, const float* g, const float* b,
                                   void* n, int64_t rows, int tokens, int d, float eps, void* stream) {
    if (int rc = pixel_op_shape("afr_op_pixel_add_ln", act_dtype, rows, d)) return rc;
    if (!h || (hin == nullptr) == (pos == nullptr)) return fail(AFR_EINVAL, "afr_op_pixel_add_ln: h and exactly one of hin / pos are required");
    if (n && (!g || !b)) return fail(AFR_EINVAL, "afr_op_pixel_add_ln: n without g, b");
    if (tokens < 1) return fail(AFR_EINVAL, "afr_op_pixel_add_ln: tokens = %d must be >= 1", tokens);
    DevGuard dg(device_of(h));
    HIPCHK(afr_launch_pixel_add_ln(act_dtype, hin, h, pos, add, g, b, n, rows, tokens, d, eps, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_pixel_attn(int act_dtype, const void* q, const void* kv, void* o, int64_t rows, int tokens, int d, int heads, int C,
                                 void* stream) {
    if (int rc = pixel_op_shape("afr_op_pixel_attn", act_dtype, rows, d)) return rc;
    if (int rc = pixel_op_attn_shape("afr_op_pixel_attn", tokens, d, heads, C)) return rc;
    if (!q || !kv || !o) return fail(AFR_EINVAL, "afr_op_pixel_attn: null argument");
    DevGuard dg(device_of(o));
    HIPCHK(afr_launch_pixel_attn(act_dtype, q, kv, o, rows, tokens, d, heads, C, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_pixel_attn_bwd(int act_dtype, const void* dO, const void* q, const void* kv, void* dq, float* dkv_part, int B, int tokens,
                                     int d, int heads, int C, void* stream) {
    if (int rc = pixel_op_shape("afr_op_pixel_attn_bwd", act_dtype, B, d)) return rc;
    if (int rc = pixel_op_attn_shape("afr_op_pixel_attn_bwd", tokens, d, heads, C)) return rc;
    if (!dO || !q || !kv || !dq || !dkv_part) return fail(AFR_EINVAL, "afr_op_pixel_attn_bwd: null argument");
    const int chunk = afr_pixel_attn_chunk(tokens);
    if ((long long)B * ((tokens + chunk - 1) / chunk) >= (1ll << 31)) return fail(AFR_EUNSUPPORTED, "afr_op_pixel_attn_bwd: B * chunks must stay below 2^31");
    DevGuard dg(device_of(dq));
    HIPCHK(afr_launch_pixel_attn_bwd(act_dtype, dO, q, kv, dq, dkv_part, B, tokens, d, C, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_pixel_head(int act_dtype, int loss_kind, const float* hin, float* h, const void* add, const float* g, const float* b,
                                 const float* w_out, const float* b_out, float* u, float* y, int64_t rows, int d, float eps, void* stream) {
    if (int rc = pixel_op_shape("afr_op_pixel_head", act_dtype, rows, d)) return rc;
    if (loss_kind != AFR_LOSS_MSE && loss_kind != AFR_LOSS_BCE) return fail(AFR_EINVAL, "afr_op_pixel_head: loss kind must be AFR_LOSS_MSE (0) or AFR_LOSS_BCE (1), got %d", loss_kind);
    if (!hin || !h || !add || !g || !b || !w_out || !b_out) return fail(AFR_EINVAL, "afr_op_pixel_head: null argument");
    DevGuard dg(device_of(h));
    HIPCHK(afr_launch_pixel_head(act_dtype, hin, h, add, g, b, w_out, b_out, u, y, rows, d, eps, (hipStream_t)stream, loss_kind));
    return AFR_OK;
}
extern "C" int afr_op_pixel_head_bwd(int act_dtype, const float* du, const float* hf, const float* g, const float* b, const float* w_out, float* dh,
                                     void* dhT, float* part, int64_t rows, int d, float eps, void* stream) {
    if (int rc = pixel_op_shape("afr_op_pixel_head_bwd", act_dtype, rows, d)) return rc;
    if (!du || !hf || !g || !b || !w_out || !dh || !part) return fail(AFR_EINVAL, "afr_op_pixel_head_bwd: null argument");
    DevGuard dg(device_of(dh));
    HIPCHK(afr_launch_pixel_head_bwd(act_dtype, du, hf, g, b, w_out, dh, dhT, part, rows, d, eps, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_pixel_ln_bwd(int act_dtype, const void* dy, const float* hin, const float* g, float* dh, void* dhT, float* part, int64_t rows,
                                   int d, float eps, void* stream) {
    if (int rc = pixel_op_shape("afr_op_pixel_ln_bwd", act_dtype, rows, d)) return rc;
    if (!dy || !hin || !g || !dh || !part) return fail(AFR_EINVAL, "afr_op_pixel_ln_bwd: null argument");
    DevGuard dg(device_of(dh));
    HIPCHK(afr_launch_pixel_ln_bwd(act_dtype, dy, hin, g, dh, dhT, part, rows, d, eps, (hipStream_t)stream));
    return AFR_OK;
}

// ---- the sheet front end's two kernels one launch each (include/afr.h): argument checks, then the launcher the plan calls
static int sheet_op_args(const char* what, int act_dtype, const afr_sheet_params* P, const int64_t* x, int ldx, int B, int L, int max_length,
                         int vocab, const afr_sheet_dropout* drop) {
    if (act_dtype != AFR_F32 && act_dtype != AFR_BF16) return fail(AFR_EINVAL, "%s: act_dtype must be AFR_F32 or AFR_BF16, got %d", what, act_dtype);
    if (B < 1) return fail(AFR_EINVAL, "%s: B = %d must be >= 1", what, B);
    if (L < 1) return fail(AFR_EINVAL, "%s: L = %d must be >= 1", what, L);
    if (max_length < 1 || vocab < 1) return fail(AFR_EINVAL, "%s: max_length = %d, vocab = %d must be >= 1", what, max_length, vocab);
    if (L > max_length) return fail(AFR_EINVAL, "%s: L = %d exceeds max_length = %d", what, L, max_length);
    if (L > 120) return fail(AFR_EUNSUPPORTED, "%s: L = %d exceeds 120 (a string's state must fit one compute unit's LDS)", what, L);
    if (ldx < L) return fail(AFR_EINVAL, "%s: ldx = %d is below L = %d", what, ldx, L);
    if ((long long)max_length * 32 >= (1ll << 31) || (long long)vocab * 32 >= (1ll << 31)) return fail(AFR_EUNSUPPORTED, "%s: a table must stay below 2^31 floats", what);
    if (!P || !x) return fail(AFR_EINVAL, "%s: null argument", what);
    if (!P->pos || !P->emb || !P->w_in || !P->b_in || !P->w_o || !P->b_o || !P->ln_g || !P->ln_b || !P->w1 || !P->b1)
        return fail(AFR_EINVAL, "%s: null parameter pointer", what);
    if (drop) {
        const float ps[3] = {drop->p_embed, drop->p_attn, drop->p_fc};
        for (float pr : ps)
            if (!(pr >= 0.f && pr < 1.f)) return fail(AFR_EINVAL, "%s: dropout rate %g outside [0, 1)", what, (double)pr);
    }
    return AFR_OK;
}
static SheetParams sheet_op_params(const afr_sheet_params* P) {
    SheetParams sp;
    sp.pos = P->pos; sp.emb = P->emb; sp.w_in = P->w_in; sp.b_in = P->b_in; sp.w_o = P->w_o; sp.b_o = P->b_o;
    sp.ln_g = P->ln_g; sp.ln_b = P->ln_b; sp.w1 = P->w1; sp.b1 = P->b1;
    return sp;
}
static SheetDrop sheet_op_drop(const afr_sheet_dropout* drop, float* save) {
    if (!drop) return sheet_drop(0, 0, 0, 0.f, 0.f, 0.f, 0, save);
    return sheet_drop(drop->seed, drop->step, drop->rank, drop->p_embed, drop->p_attn, drop->p_fc, 1, save);
}
extern "C" size_t afr_sheet_save_floats(int B, int L) {
    return B > 0 && L > 0 ? (size_t)B * (size_t)L * AFR_SHEET_SAVE_PER_POS : 0;
}
extern "C" int afr_op_sheet_fwd(int act_dtype, const afr_sheet_params* params, const int64_t* x, int ldx, int B, int L, int max_length, int vocab,
                                float ln_eps, const afr_sheet_dropout* drop, void* z, float* save, uint32_t* err, void* stream) {
    if (int rc = sheet_op_args("afr_op_sheet_fwd", act_dtype, params, x, ldx, B, L, max_length, vocab, drop)) return rc;
    if (!z) return fail(AFR_EINVAL, "afr_op_sheet_fwd: null argument");
    DevGuard dg(device_of(z));
    SheetDims d{L, max_length, 32, 4, 64, vocab};
    HIPCHK(afr_launch_sheet_fwd(act_dtype, d, sheet_op_params(params), sheet_op_drop(drop, save), x, ldx, B, z, ln_eps, err, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_sheet_bwd(int act_dtype, const afr_sheet_params* params, const int64_t* x, int ldx, int B, int L, int max_length, int vocab,
                                float ln_eps, const afr_sheet_dropout* drop, const void* dz, const float* save, float* slabs,
                                const afr_sheet_slab_layout* lay, void* stream) {
    const char* what = "afr_op_sheet_bwd";
    if (int rc = sheet_op_args(what, act_dtype, params, x, ldx, B, L, max_length, vocab, drop)) return rc;
    if (!dz || !slabs || !lay) return fail(AFR_EINVAL, "%s: null argument", what);
    if (lay->total < 4 || (lay->total & 3)) return fail(AFR_EINVAL, "%s: total = %d must be a positive multiple of 4 (a block zeroes its slab 16 bytes at a time)", what, lay->total);
    if ((uintptr_t)slabs & 15) return fail(AFR_EINVAL, "%s: slabs must be 16-byte aligned", what);
    // the ten tensor ranges lie inside a slab and do not overlap
    const long long off[10] = {lay->pos, lay->emb, lay->w_in, lay->b_in, lay->w_o, lay->b_o, lay->ln_g, lay->ln_b, lay->w1, lay->b1};
    const long long len[10] = {(long long)max_length * 32, (long long)vocab * 32, 96 * 32, 96, 32 * 32, 32, 32, 32, 64 * 32, 64};
    for (int i = 0; i < 10; ++i) {
        if (off[i] < 0 || off[i] + len[i] > lay->total) return fail(AFR_EINVAL, "%s: tensor %d (offset %lld, %lld floats) lies outside total = %d", what, i, off[i], len[i], lay->total);
        for (int j = 0; j < i; ++j)
            if (off[i] < off[j] + len[j] && off[j] < off[i] + len[i]) return fail(AFR_EINVAL, "%s: tensors %d and %d overlap", what, j, i);
    }
    DevGuard dg(device_of(slabs));
    SheetDims d{L, max_length, 32, 4, 64, vocab};
    SheetSlabOff so{lay->pos, lay->emb, lay->w_in, lay->b_in, lay->w_o, lay->b_o, lay->ln_g, lay->ln_b, lay->w1, lay->b1, lay->total};
    HIPCHK(afr_launch_sheet_bwd(act_dtype, d, sheet_op_params(params), sheet_op_drop(drop, const_cast<float*>(save)), x, ldx, B, dz, ln_eps, slabs, so,
                                (hipStream_t)stream));
    return AFR_OK;
}

// ---- the glyph nets' first-layer kernels one call each (include/afr.h): argument checks, then the launcher the plan calls
constexpr size_t GLYPH_OP_LDS_MAX = 160 * 1024;
static int glyph_op_shape(const char* what, int act_dtype, int B, int E, int vocab, int n_fonts) {
    if (act_dtype != AFR_F32 && act_dtype != AFR_BF16) return fail(AFR_EINVAL, "%s: act_dtype must be AFR_F32 or AFR_BF16, got %d", what, act_dtype);
    if (B < 1) return fail(AFR_EINVAL, "%s: B = %d must be >= 1", what, B);
    if (vocab < 1 || n_fonts < 0) return fail(AFR_EINVAL, "%s: vocab = %d, n_fonts = %d", what, vocab, n_fonts);
    if (E < 8 || E % 8) return fail(AFR_EUNSUPPORTED, "%s: E = %d must be a positive multiple of 8", what, E);
    if ((long long)(vocab + (long long)n_fonts) * E >= (1ll << 31)) return fail(AFR_EUNSUPPORTED, "%s: a table must stay below 2^31 floats", what);
    return AFR_OK;
}
static int glyph_op_n1(const char* what, int N1) {
    if (N1 < 8 || N1 % 8) return fail(AFR_EUNSUPPORTED, "%s: N1 = %d must be a positive multiple of 8", what, N1);
    return AFR_OK;
}
// the fold's post-pass stages K0 columns and E-wide rows per block (as the table + gather kernels do)
static int glyph_op_fold(const char* what, int E, int vocab, int n_fonts) {
    const long long K0 = (long long)E + ((long long)vocab + n_fonts + 7) / 8 * 8;
    if (K0 > 512 || E > 128) return fail(AFR_EUNSUPPORTED, "%s: K0 = %lld, E = %d: the folded first layer takes K0 <= 512 and E <= 128", what, K0, E);
    return AFR_OK;
}
static int glyph_op_lds(const char* what, size_t lds) {
    if (lds > GLYPH_OP_LDS_MAX) return fail(AFR_EUNSUPPORTED, "%s: %zu bytes of dynamic LDS requested, above 160 KiB", what, lds);
    return AFR_OK;
}
extern "C" int afr_op_glyph_embed(int act_dtype, const float* emb, const float* femb, const int64_t* x, const int64_t* font, int B, int E, int vocab,
                                  int n_fonts, void* out, uint32_t* err, void* stream) {
    const char* what = "afr_op_glyph_embed";
    if (int rc = glyph_op_shape(what, act_dtype, B, E, vocab, n_fonts)) return rc;
    if (!emb || !x || !out || !err || (n_fonts > 0 && !femb)) return fail(AFR_EINVAL, "%s: null argument", what);
    DevGuard dg(device_of(out));
    HIPCHK(afr_launch_glyph_embed(act_dtype, emb, femb, x, font, B, E, vocab, n_fonts, out, err, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_glyph_combo(const float* emb, const float* femb, const float* W1, const float* b1, const int64_t* x, const int64_t* font, int B,
                                  int E, int N1, int vocab, int n_fonts, void* h1c, int ld1, void* h0c, int32_t* cidx, void* w1t, uint32_t* err,
                                  void* stream) {
    const char* what = "afr_op_glyph_combo";
    if (int rc = glyph_op_shape(what, AFR_BF16, B, E, vocab, n_fonts)) return rc;
    if (int rc = glyph_op_n1(what, N1)) return rc;
    // glyph_combo_kernel keeps a W1 row of E <= 40 floats per thread in registers (the bound its 48 KiB of LDS staging used to set)
    if (E > 40) return fail(AFR_EUNSUPPORTED, "%s: E = %d is above the kernel's E <= 40 (a W1 row per thread; formerly 48 KiB of staging)", what, E);
    if (ld1 < N1) return fail(AFR_EINVAL, "%s: ld1 = %d is below N1 = %d", what, ld1, N1);
    if ((long long)vocab * (n_fonts > 0 ? n_fonts : 1) * (long long)ld1 >= (1ll << 31)) return fail(AFR_EUNSUPPORTED, "%s: the combination table must stay below 2^31 elements", what);
    if (!emb || !W1 || !b1 || !x || !h1c || !h0c || !cidx || !err || (n_fonts > 0 && !femb)) return fail(AFR_EINVAL, "%s: null argument", what);
    if ((uintptr_t)W1 & 15) return fail(AFR_EINVAL, "%s: W1 must be 16-byte aligned", what);
    DevGuard dg(device_of(h1c));
    HIPCHK(afr_launch_glyph_combo(emb, femb, W1, b1, x, font, B, E, N1, vocab, n_fonts, nullptr, h1c, ld1, h0c, cidx, err, (hipStream_t)stream, w1t));
    return AFR_OK;
}
extern "C" int afr_op_glyph_l1_bwd(const float* slabs, int nslabs, long long slab_stride, const float* W1, int N1, int E, int vocab, int n_fonts,
                                   float* dw1, float* dtab_part, void* stream) {
    const char* what = "afr_op_glyph_l1_bwd";
    if (int rc = glyph_op_shape(what, AFR_F32, 1, E, vocab, n_fonts)) return rc;
    if (int rc = glyph_op_n1(what, N1)) return rc;
    if (int rc = glyph_op_fold(what, E, vocab, n_fonts)) return rc;
    const int K0 = afr_glyph_k0(E, vocab, n_fonts);
    if (nslabs < 1) return fail(AFR_EINVAL, "%s: nslabs = %d must be >= 1", what, nslabs);
    if (slab_stride % 4 || (nslabs > 1 && slab_stride < (long long)N1 * K0))
        return fail(AFR_EINVAL, "%s: slab_stride = %lld must be a multiple of 4 and at least N1 * K0 = %lld", what, slab_stride, (long long)N1 * K0);
    if (!slabs || !W1 || !dw1 || !dtab_part) return fail(AFR_EINVAL, "%s: null argument", what);
    if ((uintptr_t)slabs & 15) return fail(AFR_EINVAL, "%s: slabs must be 16-byte aligned", what);
    const int G = std::max(1, std::min(1024 / (8 * K0 / 4), 8));                   // glyph_l1_bwd_kernel: S | W | the other lane groups' partials
    if (int rc = glyph_op_lds(what, ((size_t)8 * (K0 + E) + (size_t)(G - 1) * 8 * K0) * sizeof(float))) return rc;
    DevGuard dg(device_of(dw1));
    HIPCHK(afr_launch_glyph_l1_bwd(slabs, nslabs, slab_stride, W1, N1, E, vocab, n_fonts, dw1, dtab_part, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_glyph_l1_bwd_fused(const void* d1, const void* h0, int ldh, const int32_t* h0_rowmap, const void* W1T, const int64_t* x,
                                         const int64_t* font, int B, int N1, int vocab, int n_fonts, float* slabs, void* stream) {
    const char* what = "afr_op_glyph_l1_bwd_fused";
    if (int rc = glyph_op_shape(what, AFR_BF16, B, 32, vocab, n_fonts)) return rc;
    if (int rc = glyph_op_n1(what, N1)) return rc;
    if (!afr_glyph_l1_bwd_fused_eligible(AFR_BF16, 32, N1, vocab, n_fonts))
        return fail(AFR_EUNSUPPORTED, "%s: N1 = %d, vocab + n_fonts = %d: the fused backward takes N1 a multiple of 128 in 256 .. 1024 and at most 144 table rows (E = 32)",
                    what, N1, vocab + n_fonts);
    if (ldh < 32 || ldh % 8) return fail(AFR_EINVAL, "%s: ldh = %d must be a multiple of 8, at least 32", what, ldh);
    if ((long long)B * N1 * 2 >= (1ll << 31) || (!h0_rowmap && (long long)B * ldh * 2 >= (1ll << 31)))
        return fail(AFR_EUNSUPPORTED, "%s: d1 and h0 must stay below 2 GiB", what);
    if (!d1 || !h0 || !W1T || !x || !slabs) return fail(AFR_EINVAL, "%s: null argument", what);
    if (((uintptr_t)d1 & 15) || ((uintptr_t)h0 & 15) || ((uintptr_t)W1T & 15) || ((uintptr_t)slabs & 15))
        return fail(AFR_EINVAL, "%s: d1, h0, W1T and slabs must be 16-byte aligned", what);
    if (int rc = glyph_op_lds(what, (size_t)(N1 / afr_glyph_l1_bwd_fused_split(B, N1) / 128 + 1) * 16384 + 2 * 64 * sizeof(int))) return rc;
    DevGuard dg(device_of(slabs));
    HIPCHK(afr_launch_glyph_l1_bwd_fused(d1, N1, h0, ldh, W1T, x, font, B, N1, vocab, n_fonts, slabs, (hipStream_t)stream, h0_rowmap, nullptr));
    return AFR_OK;
}
extern "C" int afr_op_glyph_embed_bwd(int act_dtype, const void* d, const int64_t* x, const int64_t* font, int B, int E, int vocab, int n_fonts,
                                      float* slabs, void* stream) {
    const char* what = "afr_op_glyph_embed_bwd";
    if (int rc = glyph_op_shape(what, act_dtype, B, E, vocab, n_fonts)) return rc;
    if (int rc = glyph_op_lds(what, afr_glyph_embed_bwd_lds_bytes(E, vocab, n_fonts))) return rc;
    if (!d || !x || !slabs) return fail(AFR_EINVAL, "%s: null argument", what);
    DevGuard dg(device_of(slabs));
    HIPCHK(afr_launch_glyph_embed_bwd(act_dtype, d, x, font, B, E, vocab, n_fonts, slabs, (hipStream_t)stream));
    return AFR_OK;
}

// ---- the folded forward's table + gather pair, the fused step of the small glyph nets and its operand transpose, one call each
extern "C" int afr_op_glyph_l1_fwd(int act_dtype, const float* emb, const float* femb, const float* W1, const float* b1, const int64_t* x,
                                   const int64_t* font, int B, int E, int N1, int vocab, int n_fonts, float* table, void* h0p, void* h1, void* w1t,
                                   uint32_t* err, void* stream) {
    const char* what = "afr_op_glyph_l1_fwd";
    if (int rc = glyph_op_shape(what, act_dtype, B, E, vocab, n_fonts)) return rc;
    if (int rc = glyph_op_n1(what, N1)) return rc;
    if (int rc = glyph_op_fold(what, E, vocab, n_fonts)) return rc;
    if ((long long)B * std::max(N1, afr_glyph_k0(E, vocab, n_fonts)) >= (1ll << 31) || (long long)(vocab + n_fonts) * N1 >= (1ll << 31))
        return fail(AFR_EUNSUPPORTED, "%s: h1, h0' and the table must stay below 2^31 elements", what);
    if (!emb || !W1 || !b1 || !x || !table || !h0p || !h1 || !err || (n_fonts > 0 && !femb)) return fail(AFR_EINVAL, "%s: null argument", what);
    if (((uintptr_t)emb & 15) || (n_fonts > 0 && ((uintptr_t)femb & 15)) ||((uintptr_t)W1 & 15) || ((uintptr_t)b1 & 15) || ((uintptr_t)table & 15) ||
        ((uintptr_t)h0p & 15) || ((uintptr_t)h1 & 15))
        return fail(AFR_EINVAL, "%s: emb, femb, W1, b1, table, h0p and h1 must be 16-byte aligned", what);
    DevGuard dg(device_of(h1));
    HIPCHK(afr_launch_glyph_l1_fwd(act_dtype, emb, femb, W1, b1, x, font, B, E, N1, vocab, n_fonts, table, h0p, h1, err, (hipStream_t)stream, w1t));
    return AFR_OK;
}
extern "C" int afr_glyph1_blocks(int dtype, int B, int P) {
    const int R = afr_glyph1_rows(dtype);
    return B < 1 ? 0 : (B + R - 1) / R * afr_glyph1_colsplit(dtype, B, P);
}
extern "C" int afr_op_glyph1_step(int dtype, int loss_kind, const float* emb, const float* femb, const void* W1, const float* b1, const void* W2,
                                  const float* b2, const void* W1T, const void* W2T, const int64_t* x, const int64_t* font, const void* target,
                                  int target_dtype, const int32_t* target_rows, int B, int E, int N1, int P, int vocab, int n_fonts,
                                  int64_t mean_elems, float* slabs, const afr_glyph1_layout* lay, float* loss_accum, float* loss_scratch,
                                  uint32_t* err, void* stream) {
    const char* what = "afr_op_glyph1_step";
    if (dtype != AFR_F32 && dtype != AFR_BF16) return fail(AFR_EINVAL, "%s: dtype must be AFR_F32 or AFR_BF16, got %d", what, dtype);
    if (loss_kind != AFR_LOSS_MSE && loss_kind != AFR_LOSS_BCE) return fail(AFR_EINVAL, "%s: loss kind must be AFR_LOSS_MSE (0) or AFR_LOSS_BCE (1), got %d", what, loss_kind);
    if (target_dtype != AFR_TARGET_U8 && target_dtype != AFR_TARGET_F32) return fail(AFR_EINVAL, "%s: target_dtype must be AFR_TARGET_U8 or AFR_TARGET_F32, got %d", what, target_dtype);
    if (B < 1) return fail(AFR_EINVAL, "%s: B = %d must be >= 1", what, B);
    if (vocab < 1 || n_fonts < 0) return fail(AFR_EINVAL, "%s: vocab = %d, n_fonts = %d", what, vocab, n_fonts);
    if (E < 1 || N1 < 1 || P < 1) return fail(AFR_EINVAL, "%s: E = %d, N1 = %d, P = %d must be >= 1", what, E, N1, P);
    if (mean_elems < 1) return fail(AFR_EINVAL, "%s: mean_elems = %lld must be >= 1", what, (long long)mean_elems);
    if (!afr_glyph1_eligible(E, N1, P, vocab, n_fonts))
        return fail(AFR_EUNSUPPORTED, "%s: E = %d, N1 = %d, P = %d, vocab + n_fonts = %d: the fused step takes E 32 or 64, N1 and P multiples of 64 up to 256 and at most 264 table rows",
                    what, E, N1, P, vocab + n_fonts);
    if (int rc = glyph_op_lds(what, afr_glyph1_lds_bytes(dtype, E, N1, P, vocab + n_fonts))) return rc;
    const bool b16 = dtype == AFR_BF16;
    if (!emb || !W1 || !b1 || !W2 || !b2 || !x || !target || !slabs || !lay || !loss_accum || !loss_scratch || !err || (n_fonts > 0 && !femb) ||
        (b16 && (!W1T || !W2T)))
        return fail(AFR_EINVAL, "%s: null argument", what);
    if (((uintptr_t)W1 & 15) || ((uintptr_t)W2 & 15) || (b16 && (((uintptr_t)W1T & 15) || ((uintptr_t)W2T & 15))) || ((uintptr_t)slabs & 15))
        return fail(AFR_EINVAL, "%s: W1, W2, W1T, W2T and slabs must be 16-byte aligned", what);
    // the six tensor ranges lie inside a slab, start on 16 bytes and do not overlap
    if (lay->total < 4 || (lay->total & 3)) return fail(AFR_EINVAL, "%s: total = %d must be a positive multiple of 4", what, lay->total);
    const long long off[6] = {lay->emb, lay->font, lay->w1, lay->b1, lay->w2, lay->b2};
    const long long len[6] = {(long long)vocab * E, (long long)n_fonts * E, (long long)N1 * E, N1, (long long)P * N1, P};
    for (int i = 0; i < 6; ++i) {
        if (len[i] == 0) continue;
        if (off[i] < 0 || (off[i] & 3) || off[i] + len[i] > lay->total)
            return fail(AFR_EINVAL, "%s: tensor %d (offset %lld, %lld floats) must start on a multiple of 4 and lie inside total = %d", what, i, off[i], len[i], lay->total);
        for (int j = 0; j < i; ++j)
            if (len[j] && off[i] < off[j] + len[j] && off[j] < off[i] + len[i]) return fail(AFR_EINVAL, "%s: tensors %d and %d overlap", what, j, i);
    }
    DevGuard dg(device_of(slabs));
    Glyph1Args a;
    a.x = x; a.font = font;
    a.loss = loss_args(loss_scratch, true, loss_kind, target, target_dtype, target_rows, mean_elems, loss_accum);
    a.B = B; a.E = E; a.N1 = N1; a.P = P; a.vocab = vocab; a.n_fonts = n_fonts;
    a.emb = emb; a.femb = n_fonts > 0 ? femb : nullptr; a.b1 = b1; a.b2 = b2;
    a.W1 = W1; a.W2 = W2;
    a.W1T = b16 ? W1T : W1; a.W2T = b16 ? W2T : W2;                  // f32: the masters again, gathered (as the plan hands them)
    a.slabs = slabs; a.slab_stride = lay->total;
    a.o_emb = lay->emb; a.o_font = n_fonts > 0 ? lay->font : 0; a.o_w1 = lay->w1; a.o_b1 = lay->b1; a.o_w2 = lay->w2; a.o_b2 = lay->b2;
    a.err = err;
    a.cs = afr_glyph1_colsplit(dtype, B, P);
    HIPCHK(afr_launch_glyph1_step(dtype, a, (hipStream_t)stream));
    return AFR_OK;
}
extern "C" int afr_op_transpose_bf16(const float* W, void* WT, int N, int K, void* stream) {
    const char* what = "afr_op_transpose_bf16";
    if (N < 1 || K < 1) return fail(AFR_EINVAL, "%s: N = %d, K = %d must be >= 1", what, N, K);
    if (!W || !WT) return fail(AFR_EINVAL, "%s: null argument", what);
    DevGuard dg(device_of(WT));
    HIPCHK(afr_launch_transpose_bf16(W, (bf16_t*)WT, N, K, (hipStream_t)stream));
    return AFR_OK;
}
