// fwn_train_loss_and_grads: loss = -(log_p + logdet) (train.py:56-60) and its gradient with respect to every trainable
// tensor of the reference (train.py:63-66, one tf.gradients call there) for one batch, sequenced here - training forward
// with everything the backward needs kept per flow, then the flows in reverse - over the stage kernels of
// flow_kernels.hip / train_kernels.hip.  No allocation, no synchronisation: every buffer is carved from the caller's
// workspace (fwn_train_workspace_bytes), every launch goes to `stream`, so a caller may record the whole call into a
// hipGraph.  DESIGN.md section 8 describes the arithmetic; the host side (tf-flowavenet_amd/training.py) only builds the
// descriptors.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <map>
#include <vector>

#include "../../include/fwn.h"
#include "common.h"
#include "fwn_internal.h"
#include "fwn_sequence.h"

int fwn_set_error(int code, const char* fmt, ...);      // api.hip: thread-local message of fwn_last_error()
#define TREQUIRE(cond, ...) do { if (!(cond)) return fwn_set_error(FWN_ERR_ARG, __VA_ARGS__); } while (0)

namespace {

constexpr float SQH = 0.70710678118654752440f;          // sqrt(1/2), modules.py:128

// ---- small kernels that replace the host-framework tensor ops of the Python sequencing -----------------------------
__global__ __launch_bounds__(256) void scale_copy_kernel(float* __restrict__ dst, const float* __restrict__ src, long n, float s) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = (src[i] + 0.0f) * s;
}
// mel planes [2][B][T][half] -> rows [B][T][2 half]: the gradient image (fp32) and the up-sampled conditioning (bf16 -> fp32)
__global__ __launch_bounds__(256) void planes_to_rows_kernel(const float* __restrict__ dplanes, const bf16* __restrict__ cplanes,
                                                             long BT, int half, float* __restrict__ dy, float* __restrict__ y) {
    const long total = BT * 2 * half;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long bt = i / (2 * half);
        const int w = (int)(i - bt * 2 * half), q = w / half, c = w - q * half;
        const long src = ((long)q * BT + bt) * half + c;
        dy[i] = dplanes[src];
        y[i] = (float)cplanes[src];
    }
}
__global__ void up_prepare_kernel(const float* __restrict__ g, float* __restrict__ g3) {
    if (threadIdx.x < 3) g3[threadIdx.x] = g[0];        // the three kw columns share one scalar g (convolutional.py:186)
}
__global__ void up_finish_kernel(const float* __restrict__ dg3, const float* __restrict__ dwb, int s, float* __restrict__ dg,
                                 float* __restrict__ dbias) {
    if (threadIdx.x == 0) {
        dg[0] = (dg3[0] + dg3[1]) + dg3[2];
        dbias[0] = dwb[6 * s];
    }
}
__global__ void finish_loss_kernel(const float* __restrict__ out2, float* __restrict__ out3) {
    if (threadIdx.x == 0) {
        // (the tail's log-det partials carry the ActNorm terms)
        const float log_p = out2[0], logdet = out2[1];
        out3[0] = -(log_p + logdet);
        out3[1] = log_p;
        out3[2] = logdet;
    }
}
// ragged step: d loss / d z of clip b = z / (nclip len[b]) inside the clip (log_p[b] is the mean over the clip's own samples,
// the loss the mean over the clips) and 0 past its end, where the forward pass zeroed the planes.  planes [2][nclip][hT];
// a clip of len samples holds len / 2 elements of either plane.  With len = 2 hT the bits of scale_copy_kernel.
__global__ __launch_bounds__(256) void dz_init_ragged_kernel(float* __restrict__ dst, const float* __restrict__ src, long nclip, long hT,
                                                             const int* __restrict__ len) {
    const long n = 2 * nclip * hT;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long r = i / hT, b = r % nclip, k = i - r * hT;
        long L = len[b];
        L = L < 0 ? 0 : (L > 2 * hT ? 2 * hT : L);
        dst[i] = k < L / 2 ? (src[i] + 0.0f) * (float)(1.0 / ((double)nclip * (double)L)) : 0.0f;
    }
}
// out2B [2][nclip] = per-clip (log_p, logdet) -> out3 = (loss, mean log_p, mean logdet), loss = -(1/nclip) sum_b (log_p + logdet);
// fp64 sums in clip order
__global__ void finish_loss_ragged_kernel(const float* __restrict__ out2B, long nclip, float* __restrict__ out3) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double lp = 0.0, ld = 0.0;
        for (long b = 0; b < nclip; ++b) { lp += (double)out2B[b]; ld += (double)out2B[nclip + b]; }
        out3[0] = (float)(-(lp + ld) / (double)nclip);
        out3[1] = (float)(lp / (double)nclip);
        out3[2] = (float)(ld / (double)nclip);
    }
}
inline unsigned grid_of(long n) { long b = (n + 255) / 256; return (unsigned)(b > 4096 ? 4096 : (b < 1 ? 1 : b)); }

// ---- workspace carving (the same walk sizes the workspace and hands out the pointers) ------------------------------
struct Bump {
    char* base;
    size_t off = 0;
    explicit Bump(void* b) : base((char*)b) {}
    void* take(size_t bytes) {
        void* p = base ? base + off : nullptr;
        off = (off + bytes + 255) & ~(size_t)255;
        return p;
    }
};

// Fork / join markers of the side stream: created on first use (the eager first call), reused by every later call - a
// recorded call creates nothing.  One pool per host thread and device.
struct EventPool {
    std::vector<hipEvent_t> ev;
    size_t next = 0;
    hipEvent_t get() {
        if (next == ev.size()) {
            hipEvent_t e;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
            ev.push_back(e);
        }
        return ev[next++];
    }
};
EventPool* event_pool() {
    thread_local std::map<int, EventPool> pools;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    return &pools[dev];
}

struct TnSpec { int kx, n, ntap; };

// Round 4: the split count of a flow's weight-gradient GEMMs is planned for its BLOCK - with a side stream the groups of all
// n_flow flows of a block run as one launch (fwn_tn_multi_launch), and the one-stream path uses the same count so that both
// sum the same partials in the same order (bit-identical results).  `sp`: the jobs of ONE flow.
inline int tn_block_splits(const TnSpec* sp, int n, int n_flow, int m) {
    const int e = fwn_tn_tile(m);
    long tiles = 0;
    for (int i = 0; i < n; ++i) tiles += (long)sp[i].ntap * ((sp[i].kx + e - 1) / e) * ((sp[i].n + e - 1) / e);
    tiles *= n_flow;
    // the fewest splits that fill the rounds of workgroups the launch needs to 85 % (256 CUs, one 256 x 256 tile each): the
    // six flows of block 0 are 144 tiles - one split would leave 112 CUs idle, two would run a second round for 32 of them,
    // five make 720 workgroups = three rounds at 94 %
    // (few rows: the launch is bound by writing its output tiles, and every extra split is another copy of them for the
    // weight-norm backward to read - one split per tile there.  Measured per block at 8 x 6400, TN + weight-norm kernel time:
    // blocks 0-2 fill-aware 728 / 555 / 339 us against 1030 / 653 / 371 with one split; blocks 3-7 one split 261 / 239 / 283 /
    // 376 / 562 us against 287 / 236 / 302 / 422 / 672 fill-aware)
    if (m < 4096) return 1;
    const long a = (m + 63) / 64 < 32 ? (m + 63) / 64 : 32;
    for (long n = 1; n <= a; ++n) {
        const long w = tiles * n, rounds = (w + 255) / 256;
        if (100 * w >= 85 * 256 * rounds) return (int)n;
    }
    return (int)(a < 1 ? 1 : a);
}

struct FlowSaved {          // what the training forward keeps of one flow
    void* h[FWN_MAX_LAYERS]; void* o[FWN_MAX_LAYERS]; void* aux[FWN_MAX_LAYERS];
    void* s_act; void* u_act; float* z; float* part; int nb, p;
};

// Training's hoisting rule: below 4096 rows whatever cin.  Inference (api.hip, hoist_cond) also asks for cin >= 256 and
// follows cond_mode; the two differ on purpose (training runs no fragment-stream conditioning either).
static fwn_cond_plan train_cond_plan(const fwn_model_desc* md, int i, long m) {
    const fwn_flow_desc* d0 = &md->flows[i * md->n_flow];
    return fwn_plan_cond(m < 4096, (int)m, md->n_flow, md->n_layer, d0->cin, d0->kcpad, nullptr);
}

struct BwdSet { void* dz; void* du; void* ds; void* dpre[FWN_MAX_LAYERS]; void* dh[FWN_MAX_LAYERS]; void* ya_bf; double* sg; };
struct Plan {               // every buffer of one call
    void* cplanes; float* ups[FWN_MAX_UPSAMPLE]; float* planes; float* gplanes; float* dcplanes; float* P; float* Ppart;
    float* partial_all; float* out2; float* an_dummy;
    fwn_cond_plan cond[16]; // per block: the hoisted conditioning (cond[i].hoist) and its launch
    FlowSaved* saved;       // host array, owned by the caller of plan()
    // backward temporaries, sized for the largest block and reused flow after flow
    void* xhl; float* dzz; void* d_all; void* d_o[FWN_MAX_LAYERS]; float* tn_part; void* tn_table; double* wn_scratch; double* up_wn;
    // the ones the weight-gradient GEMMs read.  One set without a side stream; with one, a set per flow: its weight
    // gradients run on the side stream while the main stream goes on differentiating
    std::vector<BwdSet> sets;
    float* up_dy; float* up_y; float* up_dx[2]; float* up_dwb; float* up_scr; float* up_g3; float* up_dv; float* up_dg3;
    // ragged step only (behind everything else: the plain call's layout is untouched): the masked copy of the mel, every
    // flow's per-clip log-det sums, and the per-clip scalars where the caller wants none
    float* melc; double* acc; float* out2B;
    size_t total;
    int npart;
};

// Number of fp32 elements of the grouped weight-gradient partials of ALL flows of block i (they coexist: one launch per block).
long tn_partial_floats(const fwn_model_desc* md, int i, long m) {
    const int ch = 1 << i, L = md->n_layer, half = md->num_mels / 2, cin = half * (2 << i);
    const int ldz = 2 * ch > 8 ? 2 * ch : 8;
    TnSpec sp[4 + 5 * FWN_MAX_LAYERS];
    int n = 0;
    sp[n++] = {256, ldz, 1};
    sp[n++] = {256, 256, 1};
    for (int l = 0; l < L; ++l) sp[n++] = {256, 256, 1};
    for (int l = L - 1; l >= 0; --l) {
        if (l < L - 1) sp[n++] = {256, 256, 1};
        sp[n++] = {256, 512, 3};
        sp[n++] = {cin, 512, 1};
    }
    sp[n++] = {ch < 8 ? 8 : ch, 256, 3};
    long tot = 0;
    const int ns = tn_block_splits(sp, n, md->n_flow, (int)m);
    for (int j = 0; j < n; ++j) tot += (long)ns * ((long)sp[j].ntap * sp[j].kx + 1) * sp[j].n;
    return tot * md->n_flow;
}

// kind: PASS_TRAIN or PASS_TRAIN_RAGGED (what the ragged step adds lies behind everything else)
void plan(const fwn_train_desc* t, long B, long T, void* ws, Plan& pl, PassKind kind) {
    const fwn_model_desc* md = t->model;
    const int L = md->n_layer, half = md->num_mels / 2, nmel = 2 * half;
    Bump b(ws);
    pl.cplanes = b.take((size_t)2 * B * T * half * 2);
    long H = T / hop_of(md);
    for (int n = 0; n < md->n_up; ++n) {
        H *= md->up_scale[n];
        pl.ups[n] = n + 1 < md->n_up ? (float*)b.take((size_t)B * H * nmel * 4) : nullptr;      // output of stage n (fp32), except the last
    }
    pl.planes = (float*)b.take((size_t)B * T * 4);
    pl.gplanes = (float*)b.take((size_t)B * T * 4);
    pl.dcplanes = (float*)b.take((size_t)2 * B * T * half * 4);
    size_t pbytes = 0, ppart = 0;
    int npart = 0;
    long mmax = B * T / 2;
    for (int i = 0; i < md->n_block; ++i) {
        const long ch = 1L << i, m = B * T / (2 * ch);
        pl.cond[i] = train_cond_plan(md, i, m);
        if (pl.cond[i].hoist) {
            const size_t need = (size_t)md->n_flow * L * m * 512 * 4;
            if (need > pbytes) pbytes = need;
            const size_t sp = (size_t)(pl.cond[i].nsplit - 1) * need;
            if (sp > ppart) ppart = sp;
        }
        for (int j = 0; j < md->n_flow; ++j) {
            FlowSaved& s = pl.saved[i * md->n_flow + j];
            for (int l = 0; l < L; ++l) {
                s.h[l] = b.take((size_t)m * 256 * 2);
                s.o[l] = b.take((size_t)m * 256 * 2);
                s.aux[l] = b.take((size_t)m * 512 * 2);
            }
            s.s_act = b.take((size_t)m * 256 * 2);
            s.u_act = b.take((size_t)m * 256 * 2);
            s.z = (float*)b.take((size_t)m * 2 * ch * 4);
            {       // log-det partial slots of the flow's tail launch (in place, without a front conv)
                const fwn_flow_desc* fd = &md->flows[i * md->n_flow + j];
                s.nb = fwn_tail_slots(fwn_tail_form((int)m, fd->L, fd->Ch, fd->npt, fd->Wts != nullptr), (int)m, false);
            }
            npart += s.nb;
        }
    }
    pl.P = (float*)b.take(pbytes);
    pl.Ppart = (float*)b.take(ppart);          // split-K partials of the hoisted conditioning (few rows)
    pl.partial_all = (float*)b.take((size_t)npart * 4);
    pl.npart = npart;
    {   // partial slices in flow order
        int off = 0;
        for (int f = 0; f < md->n_block * md->n_flow; ++f) { pl.saved[f].part = pl.partial_all ? pl.partial_all + off : nullptr; off += pl.saved[f].nb; }
    }
    pl.out2 = (float*)b.take(16);
    // backward temporaries: maxima over the blocks
    size_t dz_b = 0, dzz_b = 0, ya_b = 0, tn_b = 0, wn_b = 0, sg_b = 0;
    for (int i = 0; i < md->n_block; ++i) {
        const long ch = 1L << i, m = B * T / (2 * ch), cin = (long)half * (2 << i);
        const long ldz = 2 * ch > 8 ? 2 * ch : 8;
        dz_b = dz_b > (size_t)m * ldz * 2 ? dz_b : (size_t)m * ldz * 2;
        dzz_b = dzz_b > (size_t)m * 2 * ch * 4 ? dzz_b : (size_t)m * 2 * ch * 4;
        ya_b = ya_b > (size_t)m * (ch < 8 ? 8 : ch) * 2 ? ya_b : (size_t)m * (ch < 8 ? 8 : ch) * 2;      // rows padded to 8 channels (16 bytes)
        const size_t tnb = (size_t)tn_partial_floats(md, i, m) * 4;
        tn_b = tn_b > tnb ? tn_b : tnb;
        // weight-norm scratch of a group of <= 16 jobs: bounded by the 16 largest jobs (K/32 + 1) N 2 doubles; the
        // conditioning convs dominate: (cin/32 + 1) 256 2 each; take all jobs of the flow as the bound
        size_t wn = 0;
        wn += (size_t)(256 / 32 + 1) * 256 * 2 * (1 + 2 * L);                         // final, skip, res
        wn += (size_t)(768 / 32 + 1) * 256 * 2 * 2 * L;                               // filter, gate
        wn += (size_t)(cin / 32 + 2) * 256 * 2 * 2 * L;                               // filter_c, gate_c
        wn += (size_t)(3 * ch / 32 + 2) * 256 * 2 + 64;                               // front
        wn_b = wn_b > wn * 8 ? wn_b : wn * 8;
        const size_t sg = (size_t)fwn_small_grads_blocks(m, (int)ch) * 6 * ch * 8;
        sg_b = sg_b > sg ? sg_b : sg;
    }
    pl.xhl = b.take((size_t)B * T * 2);        // front conv of the blocks with Ch >= 32: bf16 (hi | lo) image of the plane
    pl.dzz = (float*)b.take(dzz_b);
    pl.d_all = b.take((size_t)mmax * L * 256 * 2);
    for (int l = 0; l < L; ++l) pl.d_o[l] = b.take((size_t)mmax * 256 * 2);
    // one set per flow with a side stream (a set stays live until its block is joined), sized for the flow's block
    const int nsets = t->side_stream ? md->n_block * md->n_flow : 1;
    pl.sets.resize(nsets);
    for (int k = 0; k < nsets; ++k) {
        const long mset = t->side_stream ? B * T / (2L << (k / md->n_flow)) : mmax;
        BwdSet& w = pl.sets[k];
        w.dz = b.take(dz_b);
        w.du = b.take((size_t)mset * 256 * 2);
        w.ds = b.take((size_t)mset * 256 * 2);
        for (int l = 0; l < L; ++l) {
            w.dpre[l] = b.take((size_t)mset * 512 * 2);
            w.dh[l] = b.take((size_t)mset * 256 * 2);
        }
        w.ya_bf = b.take(ya_b);
        w.sg = (double*)b.take(sg_b);          // row-range partials of the flow's small gradients (totalled on the side stream)
    }
    pl.tn_part = (float*)b.take(tn_b);
    pl.tn_table = b.take(fwn_tn_table_bytes());       // group tables of the block-wide weight-gradient launch
    pl.wn_scratch = (double*)b.take(wn_b);
    pl.up_wn = (double*)b.take(1024 * 8);
    // up-sampling backward
    pl.up_dy = (float*)b.take((size_t)B * T * nmel * 4);
    pl.up_y = (float*)b.take((size_t)B * T * nmel * 4);
    int smax = 2;
    for (int n = 0; n < md->n_up; ++n) smax = md->up_scale[n] > smax ? md->up_scale[n] : smax;
    for (int k = 0; k < 2; ++k) { pl.up_dx[k] = (float*)b.take((size_t)B * (T / md->up_scale[md->n_up - 1]) * nmel * 4); }
    pl.up_dwb = (float*)b.take((size_t)(6 * smax + 1) * 4);
    pl.up_scr = (float*)b.take((size_t)64 * (6 * smax + 1) * 4);
    pl.up_g3 = (float*)b.take(16);
    pl.up_dv = (float*)b.take((size_t)2 * smax * 3 * 4);
    pl.up_dg3 = (float*)b.take(16);
    if (pass_traits(kind).ragged) {
        pl.melc = (float*)b.take((size_t)B * (T / hop_of(md)) * nmel * 4);
        pl.acc = (double*)b.take((size_t)md->n_block * md->n_flow * B * fwn_ragged_logdet_nslot(B) * 8);
        pl.out2B = (float*)b.take((size_t)2 * B * 4);
    }
    pl.total = b.off;
}

// ---- fwn_gemm descriptors (the keyword arguments of training.gemm) ---------------------------------------------------
struct Seg { const void* x; long rows; int ld, k, shift, koff; };
fwn_gemm_desc gemm_desc(const Seg* segs, int nseg, const void* W, int ldw, int N, long M, int Ti, void* Y, int ldy, bool out_f32) {
    fwn_gemm_desc d;
    memset(&d, 0, sizeof(d));
    for (int s = 0; s < nseg; ++s) {
        d.seg[s].x = segs[s].x; d.seg[s].rows = (int)segs[s].rows; d.seg[s].ld = segs[s].ld; d.seg[s].k = segs[s].k;
        d.seg[s].shift = segs[s].shift; d.seg[s].koff = segs[s].koff;
    }
    d.nseg = nseg; d.M = (int)M; d.N = N; d.Ti = Ti;
    d.W = W; d.ldw = ldw;
    d.Y = Y; d.ldy = ldy; d.out_f32 = out_f32 ? 1 : 0;
    d.nsplit = 1; d.oscale = 1.0f;
    return d;
}

struct TnList {
    fwn_tn_job job[4 + 5 * FWN_MAX_LAYERS];
    int n = 0;
    int add(const void* x, int ldx, const void* dy, int ldy, int kx, int N, int ntap, int shift0, int dshift) {
        fwn_tn_job& q = job[n];
        memset(&q, 0, sizeof(q));
        q.x = x; q.dy = dy; q.ldx = ldx; q.Kx = kx; q.ntap = ntap; q.shift0 = shift0; q.dshift = dshift; q.ldy = ldy; q.N = N; q.bias_row = 1;
        return n++;
    }
};
struct WnItem { int tn; const float* part_direct; int part_nsplit; long part_stride; int part_rows, part_ld;   // tn < 0: part_direct
                 const fwn_conv_grad* c; int k, n, col0; float scale; const int32_t* row_src; const int32_t* col_src; };
// The weight gradients of one flow, collected by its data-gradient chain and enqueued behind it (or on the side stream)
struct Deferred {
    TnList tn; WnItem wn[4 + 7 * FWN_MAX_LAYERS]; int nwn; long m, ti; int ch, i; const BwdSet* w;
    const fwn_flow_train_desc* td;
    const float* an;                                   // the flow's ActNorm table (totals of the small gradients)
    fwn_gemm_desc dca[FWN_MAX_LAYERS]; int ndca;      // conditioning-gradient GEMMs (accumulate into the mel image: order kept)
    void add_wn(int tnj, const fwn_conv_grad* c, int k, int n, int col0, float scale, const int32_t* row_src, const int32_t* col_src) {
        wn[nwn++] = WnItem{tnj, nullptr, 0, 0, 0, 0, c, k, n, col0, scale, row_src, col_src};
    }
};

// NULL: a step can run this model at (B, T); else what is wrong with the shape (the workspace queries answer 0 there)
const char* shape_error(const fwn_model_desc* md, long B, long T) {
    if (!(md->n_block >= 1 && md->n_block <= 16 && md->n_flow >= 1 && md->n_block * md->n_flow <= 256 && md->n_layer >= 1 &&
          md->n_layer <= FWN_MAX_LAYERS))
        return "bad n_block / n_flow / n_layer";
    if (!(B > 0 && T > 0 && T % hop_of(md) == 0 && T % (1L << md->n_block) == 0)) return "T must be a multiple of hop_size and 2^n_block";
    return nullptr;
}

size_t train_workspace(const fwn_train_desc* t, int64_t B, int64_t T, PassKind kind) {
    if (!t || !t->model || !t->flows || shape_error(t->model, (long)B, (long)T)) return 0;
    FlowSaved saved[256];
    Plan pl{};
    pl.saved = saved;
    plan(t, (long)B, (long)T, nullptr, pl, kind);
    return pl.total;
}

// One call of either entry point: what its phases share, and one member function per phase - run() is the sequence.
// len (ragged step): the clips' lengths on the device - the forward half then runs the fills of the ragged forward pass
// (fwn_sequence.h: the walks inference runs) and the backward half their adjoint: where the forward overwrote rows with a
// constant, the gradient arriving at those rows is dropped.  out2B: per-clip scalars (NULL: kept in the workspace).
struct TrainCall {
    // ---- the arguments ----
    PassKind kind;
    const fwn_train_desc* t;
    long B, T;
    const float* x; const float* mel; const int32_t* len;
    void* workspace; size_t workspace_bytes;
    float* out3; float* out2B;
    fwn_block_done_fn on_block_done; void* user;
    hipStream_t st;
    // ---- set by prepare() ----
    const fwn_model_desc* md = nullptr;
    int L = 0, half = 0, nmel = 0, NF = 0;
    size_t plane_elems = 0, cplane_elems = 0;
    ClipRows rows{nullptr, 0, nullptr};
    Plan pl{};
    FlowSaved saved[256];
    // ---- the side stream (backward) ----
    hipStream_t side = nullptr;
    EventPool* evp = nullptr;
    std::vector<Deferred> pending;        // the flows of the block whose weight gradients are still to be enqueued
    int pending_block = -1;               // block whose weight gradients run on the side stream, not yet joined
    bool hook_failed = false;             // a hook that returns non-zero stops the sequencing where it stands (the side stream is joined at that point)
    hipEvent_t dca_done = nullptr;        // side stream, block 0: behind the last conditioning-gradient GEMM of the call
    bool forked = false;                  // something has been handed to the side stream and run() has not ended in FWN_OK

    // What one flow's backward works on
    struct FlowCtx {
        int i, j, ch, cin, ldz; long ti, m;
        const fwn_flow_desc* d; const fwn_flow_train_desc* td; const FlowSaved* s; const BwdSet* w;
        float* xa; float* xb;              // y_a, out_b
        float* ga; float* gb;
        const void* ca; float* dca;
    };

    // Error exits: once anything has been handed to the side stream, EVERY return path joins it into `st` first -
    // otherwise weight-gradient kernels of the block handed over last would keep reading and writing the caller's workspace
    // and gradient buffers after the call has returned an error.  Event-based, so it is also legal while the stream is being
    // captured.
    ~TrainCall() {
        if (!forked || !side || !evp) return;
        hipEvent_t e = evp->get();
        if (!e || hipEventRecord(e, side) != hipSuccess || hipStreamWaitEvent(st, e, 0) != hipSuccess) (void)hipStreamSynchronize(side);
    }

    int run() {
        int rc = prepare();
        if (rc != FWN_OK) return rc;
        rc = forward();
        if (rc != FWN_OK) return rc;
        finish_loss();
        rc = backward();
        if (rc != FWN_OK) return rc;
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fwn_set_error(FWN_ERR_HIP, "fwn_train_loss_and_grads: %s", hipGetErrorString(e));
        forked = false;                   // every block was joined on the way (join_pending)
        return FWN_OK;
    }

    // ---------------- argument checks and planning ----------------
    int prepare() {
        TREQUIRE(t && t->model && t->flows && t->model->flows, "fwn_train_loss_and_grads: null descriptor");
        TREQUIRE(x && mel && workspace && out3, "fwn_train_loss_and_grads: null pointer");
        TREQUIRE((((uintptr_t)workspace) & 255) == 0, "fwn_train_loss_and_grads: workspace must be 256-byte aligned");
        md = t->model;
        L = md->n_layer; half = md->num_mels / 2; nmel = 2 * half; NF = md->n_flow;
        const char* bad = shape_error(md, B, T);
        TREQUIRE(!bad, "fwn_train_loss_and_grads: %s", bad);
        TREQUIRE((int64_t)L * (B * T / 2) * 512 < ((int64_t)1 << 31), "fwn_train_loss_and_grads: B*T too large (2 GiB per activation buffer)");
        for (int i = 0; i < md->n_block; ++i)
            TREQUIRE(t->cond_rows[i] && t->front_rows[i] && t->zinv32[i] && t->br[i] && t->zcol[i], "fwn_train_loss_and_grads: missing index table (block %d)", i);
        TREQUIRE(!len || !md->gate_fp8, "fwn_train_loss_and_grads_ragged: per-clip lengths go with a model without fp8 gates (its e4m3 copies of h are not masked)");
        TREQUIRE(!len || B < 32768, "fwn_train_loss_and_grads_ragged: B=%ld clips (at most 32767 per call)", B);
        pl.saved = saved;
        plan(t, B, T, workspace, pl, kind);
        if (workspace_bytes < pl.total) return fwn_set_error(FWN_ERR_WORKSPACE, "workspace %zu < required %zu bytes", workspace_bytes, pl.total);
        plane_elems = (size_t)B * T / 2;
        cplane_elems = (size_t)B * T * half;
        rows = ClipRows{len, B, st};
        return FWN_OK;
    }

    // ---------------- forward, keeping what the backward needs ----------------
    int forward() {
        {   // ragged: the up-sampling backward reads the masked buffers of this walk
            UpsampleBufs u;
            memset(&u, 0, sizeof(u));
            u.mel_copy = pl.melc;
            for (int n = 0; n < md->n_up; ++n) {
                TREQUIRE(t->up_bias_dev[n], "fwn_train_loss_and_grads: up_bias_dev[%d] is null", n);
                u.inner[n] = pl.ups[n];
            }
            u.cplanes = pl.cplanes;
            u.bias_dev = t->up_bias_dev;
            if (fwn_run_upsample(md, B, T, mel, u, rows)) return fwn_set_error(FWN_ERR_HIP, "fwn_train_loss_and_grads_ragged: mel copy failed");
        }
        fwn_launch_split(x, B, T, pl.planes, st);
        // ragged: both planes hold clip b's samples at [b][0, len / 2) at every block; the rest is zeroed here and behind every flow
        rows.zero_planes(pl.planes, T);
        const int nslot = len ? fwn_ragged_logdet_nslot(B) : 0;
        int p = 0;
        for (int i = 0; i < md->n_block; ++i) {
            const int ch = 1 << i;
            const long ti = T / (2 * ch), m = B * ti;
            const int cin = half * (2 << i);
            const fwn_flow_desc* d0 = &md->flows[i * NF];
            const bool hoist = pl.cond[i].hoist;
            if (hoist)
                fwn_run_cond(pl.cond[i], (const bf16*)pl.cplanes + (size_t)p * cplane_elems, (const bf16*)pl.cplanes + (size_t)(p ^ 1) * cplane_elems,
                             d0->Wc[0], pl.P, pl.Ppart, (int)m, NF, L, cin, d0->kcpad, st);
            for (int j = 0; j < NF; ++j) {
                const fwn_flow_desc* d = &md->flows[i * NF + j];
                FlowSaved& s = saved[i * NF + j];
                s.p = p;
                float* xa = pl.planes + (size_t)p * plane_elems;
                float* xb = pl.planes + (size_t)(p ^ 1) * plane_elems;
                const void* ca = (const bf16*)pl.cplanes + (size_t)p * cplane_elems;
                // the inference kernels, keeping what the backward needs: the front conv applies the flow's ActNorm on the fly, the
                // tail (skip sum -> final conv -> ZeroConv -> coupling + ActNorm of both planes, csrc/tail_chain.h) leaves
                // y_a / out_b in the planes - the state the backward starts from - and writes S, U and Z on its way.
                // The stages over the buffers kept per layer: no fp8, no gate stream, the bf16 (hi | lo) image as the front
                // conv's scratch from Ch >= 32
                FlowStages sg;
                memset(&sg, 0, sizeof(sg));
                for (int l = 0; l < L; ++l) { sg.h[l] = s.h[l]; sg.o[l] = s.o[l]; sg.aux[l] = s.aux[l]; }
                sg.front_scratch = ch >= 32 ? pl.xhl : nullptr;
                fwn_run_stages(d, sg, xa, hoist ? nullptr : ca, hoist ? pl.P + (size_t)j * L * m * 512 : nullptr, (int)m, (int)ti, 0, rows);
                const int rc = tail(d, s, xa, xb, m, ch);
                if (rc != FWN_OK) return rc;
                if (len) {      // per-clip log-det sums from the Z the tail keeps for the backward (its own whole-batch partials are ignored)
                    fwn_launch_range_logdet(s.z, B, ti, ch, d->ezero, d->an, nullptr, len, (int)B, 2 * ch, pl.acc + (size_t)(i * NF + j) * B * nslot, st);
                    rows.zero_planes(pl.planes, T);
                }
                p ^= 1;
            }
        }
        return FWN_OK;
    }
    int tail(const fwn_flow_desc* d, const FlowSaved& s, float* xa, float* xb, long m, int ch) {
        const long o_stride = L > 1 ? (long)(((const char*)s.o[1] - (const char*)s.o[0]) / 2) : 0;
        for (int l = 1; l < L; ++l)
            TREQUIRE((const char*)s.o[l] == (const char*)s.o[0] + (size_t)l * o_stride * 2, "fwn_train_loss_and_grads: o buffers not evenly spaced");
        // the tail addresses o through ONE 32-bit buffer descriptor (byte span of all L layers, as fwn_tail_train checks)
        TREQUIRE(((long)(L - 1) * o_stride + m * 256) * 2 < (1L << 31), "fwn_train_loss_and_grads: o rows of a flow span %ld bytes: beyond the tail's 32-bit buffer offsets", ((long)(L - 1) * o_stride + m * 256) * 2);
        fwn_tail_chain tc;
        memset(&tc, 0, sizeof(tc));
        tc.save_s = s.s_act; tc.save_u = s.u_act; tc.save_z = s.z;
        fwn_launch_tail(s.o[0], o_stride, L, d->Wskip, d->bskip, d->Wfinal, d->bfinal, d->Wzero, d->bzero, d->ezero, d->an, xa, xb, s.part,
                        (int)m, ch, d->npt, 0, nullptr, nullptr, &tc, d->Wts, st);
        return FWN_OK;
    }

    // ---------------- the loss ----------------
    void finish_loss() {
        if (len) {
            float* o2 = out2B ? out2B : pl.out2B;
            fwn_launch_ragged_finish(pl.planes, B, T, pl.acc, md->n_block * NF, NF, len, o2, st);
            hipLaunchKernelGGL(finish_loss_ragged_kernel, dim3(1), dim3(64), 0, st, (const float*)o2, B, out3);
        } else {
            fwn_launch_prior(pl.planes, B * T, pl.partial_all, pl.npart, 1.0 / (double)(B * T), pl.out2, st);
            hipLaunchKernelGGL(finish_loss_kernel, dim3(1), dim3(64), 0, st, pl.out2, out3);
        }
    }

    // ---------------- backward ----------------
    // The data gradients of a flow are one dependent chain of small launches; its weight gradients (grouped TN GEMM,
    // weight-norm backward) and the conditioning gradient hang off that chain and nothing on it waits for them.  With
    // t->side_stream they run there, block by block: block i's under the main stream's chain through block i - 1, joined
    // before on_block_done(i).  Measured alternatives, all slower: handing over flow by flow (every fork / join is a
    // cross-queue edge), issuing a block's side launches one flow at a time between the next chain's flows, never
    // joining before the end.  The two queues overlap only partly (tools/diag/train_timeline.py: a chain launch of a few
    // workgroups waits behind the dispatch of a side kernel that fills the chip - tools/probe/queue_overlap.hip).
    // Without a side stream they follow their flow on the one stream.
    int backward() {
        side = (hipStream_t)t->side_stream;
        if (side) {
            evp = event_pool();
            TREQUIRE(evp, "fwn_train_loss_and_grads: hipEventCreate failed");
            evp->next = 0;
        }
        // d loss / d z = z / (B T)   (log_p = mean 0.5 (-log 2 pi - z^2))
        if (len) hipLaunchKernelGGL(dz_init_ragged_kernel, dim3(grid_of(B * T)), dim3(256), 0, st, pl.gplanes, (const float*)pl.planes, B, T / 2, len);
        else hipLaunchKernelGGL(scale_copy_kernel, dim3(grid_of(B * T)), dim3(256), 0, st, pl.gplanes, pl.planes, B * T, (float)(1.0 / (double)(B * T)));
        if (hipMemsetAsync(pl.dcplanes, 0, (size_t)2 * B * T * half * 4, st) != hipSuccess) return fwn_set_error(FWN_ERR_HIP, "hipMemsetAsync failed");
        for (int i = md->n_block - 1; i >= 0; --i)
            for (int j = NF - 1; j >= 0; --j) {
                const int rc = flow_backward(i, j);
                if (rc != FWN_OK) return rc;
            }
        // The conditioning gradient is complete behind stage (1) of block 0's weight gradients (side stream): the up-sampling
        // backward waits for THAT event and runs under the rest of block 0's side work (its grouped TN GEMM and weight-norm
        // backward: ~1 ms in which the chain's queue had nothing to do); block 0 is joined and reported behind it.
        if (side && dca_done) {
            if (hipStreamWaitEvent(st, dca_done, 0) != hipSuccess) return fwn_set_error(FWN_ERR_HIP, "fwn_train_loss_and_grads: hipStreamWaitEvent failed");
        } else if (side) {
            if (!join_pending()) return fwn_set_error(FWN_ERR_HIP, "fwn_train_loss_and_grads: joining the side stream failed");
            if (hook_failed) return hook_stop();
        }
        const int rc = upsample_backward();
        if (rc != FWN_OK) return rc;
        if (side && !join_pending()) return fwn_set_error(FWN_ERR_HIP, "fwn_train_loss_and_grads: joining the side stream failed");
        if (hook_failed) return hook_stop();
        if (on_block_done && on_block_done(user, -1) != 0) return hook_stop();
        return FWN_OK;
    }
    int hook_stop() { return fwn_set_error(FWN_ERR_CALLBACK, "fwn_train_loss_and_grads: the on_block_done callback asked to stop"); }

    // One flow: its data-gradient chain, and where its weight gradients go - behind the chain's front-conv job on the one
    // stream, or with its block's to the side stream once the block's first flow is through
    int flow_backward(int i, int j) {
        const FlowCtx F = flow_ctx(i, j);
        pending.emplace_back();
        Deferred& D = pending.back();
        D.nwn = 0; D.m = F.m; D.ti = F.ti; D.ch = F.ch; D.i = i; D.w = F.w; D.td = F.td; D.ndca = 0; D.an = F.d->an;
        chain_to_skip(F, D);
        int rc = chain_layers(F, D);
        if (rc != FWN_OK) return rc;
        rc = chain_front(F, D);
        if (rc != FWN_OK) return rc;
        if (!side) {
            rc = weight_grads(D, st);
            if (rc != FWN_OK) return rc;
            pending.clear();
        }
        rc = chain_end(F);
        if (rc != FWN_OK) return rc;
        if (!side) fwn_small_grads_final(F.d->an, F.m, F.ch, (const long long*)t->br[i], (const long long*)t->zcol[i], F.w->sg, F.td->d_an_b,
                                         F.td->d_an_logs, F.td->d_zscale, st);
        if (!side && j == 0 && on_block_done && on_block_done(user, i) != 0) hook_failed = true;
        if (hook_failed) return hook_stop();
        if (side && j == 0) {      // this block's weight gradients: under the next block's chain
            if (!join_pending()) return fwn_set_error(FWN_ERR_HIP, "fwn_train_loss_and_grads: joining the side stream failed");
            if (hook_failed) return hook_stop();
            rc = hand_over(i == 0);
            if (rc != FWN_OK) return rc;
            pending_block = i;
        }
        return FWN_OK;
    }
    FlowCtx flow_ctx(int i, int j) const {
        FlowCtx F;
        F.i = i; F.j = j; F.ch = 1 << i;
        F.ti = T / (2 * F.ch); F.m = B * F.ti;
        F.cin = half * (2 << i);
        F.ldz = 2 * F.ch > 8 ? 2 * F.ch : 8;
        F.d = &md->flows[i * NF + j];
        F.td = &t->flows[i * NF + j];
        F.s = &saved[i * NF + j];
        F.w = side ? &pl.sets[(size_t)i * NF + j] : &pl.sets[0];
        const int pp = F.s->p;
        F.xa = pl.planes + (size_t)pp * plane_elems;
        F.xb = pl.planes + (size_t)(pp ^ 1) * plane_elems;
        F.ga = pl.gplanes + (size_t)pp * plane_elems;
        F.gb = pl.gplanes + (size_t)(pp ^ 1) * plane_elems;
        F.ca = (const bf16*)pl.cplanes + (size_t)pp * cplane_elems;
        F.dca = pl.dcplanes + (size_t)pp * cplane_elems;
        return F;
    }
    // nothing in the flow chain reads the conditioning gradient: with a side stream it leaves the chain
    void cond_grad(Deferred& D, const fwn_gemm_desc& g) {
        if (side) D.dca[D.ndca++] = g;
        else fwn_gemm_launch(&g, st);
    }

    // ---- the data-gradient chain of one flow (all on `st`), collecting the flow's weight-gradient jobs in D ----
    // coupling -> ZeroConv -> final conv -> the skip convs of every layer
    void chain_to_skip(const FlowCtx& F, Deferred& D) {
        const FlowSaved& s = *F.s;
        const BwdSet& w = *F.w;
        const fwn_flow_train_desc* td = F.td;
        const long m = F.m;
        const int ch = F.ch, ldz = F.ldz;
        TnList& tn = D.tn;
        // coupling
        // (also: the bf16 copy of y_a for the front conv's weight gradient, and the zero padding of dZ's rows)
        if (len) fwn_ew_coupling_bwd_ragged(F.gb, F.xb, s.z, td->ez, B, F.ti, ch, len, 2 * ch, w.dz, ldz, pl.dzz, F.xa, w.ya_bf, ch < 8 ? 8 : ch, st);
        else fwn_ew_coupling_bwd_ex(F.gb, F.xb, s.z, td->ez, m * ch, ch, (float)(1.0 / (2.0 * (double)m * ch)), w.dz, ldz, pl.dzz, F.xa, w.ya_bf, ch < 8 ? 8 : ch, st);
        {
            Seg a{w.dz, m, ldz, ldz, 0, 0};
            fwn_gemm_desc g = gemm_desc(&a, 1, td->WzT, ldz, 256, m, 0, w.du, 256, false);
            g.mask = s.u_act; g.ldmask = 256;
            fwn_gemm_launch(&g, st);
        }
        D.add_wn(tn.add(s.u_act, 256, w.dz, ldz, 256, ldz, 1, 0, 0), &td->zero, 256, 2 * ch, 0, 1.0f, nullptr, t->zinv32[F.i]);
        D.add_wn(tn.add(s.s_act, 256, w.du, 256, 256, 256, 1, 0, 0), &td->final_, 256, 256, 0, 1.0f, nullptr, nullptr);
        {
            Seg a{w.du, m, 256, 256, 0, 0};
            fwn_gemm_desc g = gemm_desc(&a, 1, td->WfinT, 256, 256, m, 0, w.ds, 256, false);
            g.mask = s.s_act; g.ldmask = 256;
            fwn_gemm_launch(&g, st);
            Seg a2{w.ds, m, 256, 256, 0, 0};
            g = gemm_desc(&a2, 1, td->WskipT_all, 256, L * 256, m, 0, pl.d_all, L * 256, false);      // do_l = dS Wskip_l for every layer at once
            // the last layer's do is complete here: its gate derivative rides this epilogue (no store + fwn_gate_bwd)
            g.gate_aux = s.aux[L - 1]; g.gate_out = w.dpre[L - 1]; g.gate_col0 = (L - 1) * 256;
            fwn_gemm_launch(&g, st);
        }
        for (int l = 0; l < L; ++l) D.add_wn(tn.add(s.o[l], 256, w.ds, 256, 256, 256, 1, 0, 0), &td->skip[l], 256, 256, 0, 1.0f, nullptr, nullptr);
    }
    // the layers, last first: res conv -> gate -> dilated conv (and the layer's conditioning gradient); leaves dh_0 in w.dh[0]
    int chain_layers(const FlowCtx& F, Deferred& D) {
        const FlowSaved& s = *F.s;
        const BwdSet& w = *F.w;
        const fwn_flow_train_desc* td = F.td;
        const long m = F.m;
        const int cin = F.cin;
        TnList& tn = D.tn;
        const void* dh_next = nullptr;
        for (int l = L - 1; l >= 0; --l) {
            const int dil = dilation_of(l);
            const void* d_ol = (const bf16*)pl.d_all + (size_t)l * 256;
            int ld_do = L * 256;
            if (dh_next) {      // h_{l+1} = (h_l + res(o_l)) sqrt(1/2)
                D.add_wn(tn.add(s.o[l], 256, dh_next, 256, 256, 256, 1, 0, 0), &td->res[l], 256, 256, 0, SQH, nullptr, nullptr);
                Seg a{dh_next, m, 256, 256, 0, 0};
                fwn_gemm_desc g = gemm_desc(&a, 1, td->WresT[l], 256, 256, m, 0, pl.d_o[l], 256, false);
                g.R = d_ol; g.ldr = ld_do; g.rscale = (float)(1.0 / 0.7071067811865476); g.oscale = SQH;
                g.gate_aux = s.aux[l]; g.gate_out = w.dpre[l]; g.gate_col0 = 0;      // do_l goes straight through the gate derivative
                fwn_gemm_launch(&g, st);
            } else if (t->zero_dead_res) {      // dead res_conv of the last layer (modules.py:126-128): zero gradients
                const fwn_conv_grad& c = td->res[l];
                if (c.dV && hipMemsetAsync(c.dV, 0, (size_t)256 * 256 * 4, st) != hipSuccess) return fwn_set_error(FWN_ERR_HIP, "hipMemsetAsync failed");
                if (c.dg && hipMemsetAsync(c.dg, 0, 256 * 4, st) != hipSuccess) return fwn_set_error(FWN_ERR_HIP, "hipMemsetAsync failed");
                if (c.db && hipMemsetAsync(c.db, 0, 256 * 4, st) != hipSuccess) return fwn_set_error(FWN_ERR_HIP, "hipMemsetAsync failed");
            }
            const int jd = tn.add(s.h[l], 256, w.dpre[l], 512, 256, 512, 3, -dil, dil);
            D.add_wn(jd, &td->filt[l], 768, 256, 0, 1.0f, nullptr, nullptr);
            D.add_wn(jd, &td->gate[l], 768, 256, 256, 1.0f, nullptr, nullptr);
            const int jc = tn.add(F.ca, cin, w.dpre[l], 512, cin, 512, 1, 0, 0);
            D.add_wn(jc, &td->filt_c[l], cin, 256, 0, 1.0f, t->cond_rows[F.i], nullptr);
            D.add_wn(jc, &td->gate_c[l], cin, 256, 256, 1.0f, t->cond_rows[F.i], nullptr);
            if (td->wct_ld != L * 512) {        // (else the layers' WcT lie side by side: one GEMM behind the loop, chain_front)
                Seg a{w.dpre[l], m, 512, 512, 0, 0};
                fwn_gemm_desc g = gemm_desc(&a, 1, td->WcT[l], td->wct_ld ? td->wct_ld : 512, cin, m, 0, F.dca, cin, true);
                g.accumulate = 1;
                cond_grad(D, g);
            }
            Seg sg[3];
            for (int tap = 0; tap < 3; ++tap) sg[tap] = {w.dpre[l], m, 512, 512, -(tap - 1) * dil, tap * 512};
            fwn_gemm_desc g = gemm_desc(sg, 3, td->WdT[l], 1536, 256, m, (int)F.ti, w.dh[l], 256, false);
            if (dh_next) { g.R = dh_next; g.ldr = 256; g.rscale = SQH; }
            if (l == 0) { g.mask = s.h[0]; g.ldmask = 256; }
            // ragged: the forward zeroed h_l past each clip's end, so dh_l is stored as 0 there (in this launch's epilogue)
            if (len) { g.row_len = len; g.len_spr = 2 * F.ch; }
            fwn_gemm_launch(&g, st);
            dh_next = w.dh[l];
        }
        return FWN_OK;
    }
    // the flow's conditioning gradient where it is one GEMM, and the front conv's weight-gradient job
    int chain_front(const FlowCtx& F, Deferred& D) {
        const BwdSet& w = *F.w;
        const fwn_flow_train_desc* td = F.td;
        const int ch = F.ch;
        if (td->wct_ld == L * 512) {      // conditioning gradient of the flow: dca += [dpre_0 | dpre_1 | ..] [Wc_0 ; Wc_1 ; ..]
            Seg sg[FWN_MAX_LAYERS];
            for (int l = 0; l < L; ++l) {
                TREQUIRE((const char*)td->WcT[l] == (const char*)td->WcT[0] + (size_t)l * 512 * 2, "fwn_train_loss_and_grads: wct_ld = L*512 needs WcT[l] = WcT[0] + l*512");
                sg[l] = {w.dpre[l], F.m, 512, 512, 0, l * 512};
            }
            fwn_gemm_desc g = gemm_desc(sg, L, td->WcT[0], L * 512, F.cin, F.m, 0, F.dca, F.cin, true);
            g.accumulate = 1;
            cond_grad(D, g);
        }
        // front conv: y_a rows are padded to 8 channels (16 bytes: the unit the TN GEMM moves), so every block's front weight
        // gradient is one more job of the group; front_rows maps logical row tap Ch + c to GEMM row tap max(Ch, 8) + c'
        const int kxp = ch < 8 ? 8 : ch;
        D.add_wn(D.tn.add(w.ya_bf, kxp, w.dh[0], 256, kxp, 256, 3, -1, 1), &td->front, 3 * ch, 256, 0, 1.0f, t->front_rows[F.i], nullptr);
        return FWN_OK;
    }
    // front conv's data gradient, then ActNorm of both planes back to the flow's inputs, with the row-range partials of its
    // b / logs gradients and of the ZeroConv scale gradient
    int chain_end(const FlowCtx& F) {
        const fwn_flow_train_desc* td = F.td;
        {
            Seg sg[3];
            for (int tap = 0; tap < 3; ++tap) sg[tap] = {F.w->dh[0], F.m, 256, 256, -(tap - 1), tap * 256};
            fwn_gemm_desc g = gemm_desc(sg, 3, td->WfT, 768, F.ch, F.m, (int)F.ti, F.ga, F.ch, true);
            g.accumulate = 1;
            fwn_gemm_launch(&g, st);
        }
        TREQUIRE(td->d_an_b && td->d_an_logs && td->d_zscale, "fwn_train_loss_and_grads: flow (%d,%d): missing small gradient pointers", F.i, F.j);
        if (len) fwn_small_grads_main_ragged(F.ga, F.xa, F.gb, F.xb, pl.dzz, F.d->an, B, F.ti, F.ch, len, 2 * F.ch, F.w->sg, st);
        else fwn_small_grads_main(F.ga, F.xa, F.gb, F.xb, pl.dzz, F.d->an, F.m, F.ch, F.w->sg, st);
        return FWN_OK;
    }

    // ---- the weight gradients of a flow in three stages: (1) totals of the small gradients + the conditioning-gradient GEMMs,
    // (2) the grouped TN GEMM(s) into fp32 partials, (3) the grouped weight-norm backward(s) that total them.  One stream:
    // (1)-(3) behind the flow's chain.  Side stream: (1) of every flow of the block, then (2) of ALL its flows as ONE launch
    // (fwn_tn_multi_launch: the block fills the chip with a sixth of the splits a flow on its own would need - a sixth of the
    // partials to write and to read back), then (3) flow by flow.  `part`: where the flow's partials go (advanced).
    void wg_small(Deferred& D, hipStream_t s_) {
        if (side)       // (one stream: totalled right behind their first pass, on the chain)
            fwn_small_grads_final(D.an, D.m, D.ch, (const long long*)t->br[D.i], (const long long*)t->zcol[D.i], D.w->sg, D.td->d_an_b, D.td->d_an_logs,
                                  D.td->d_zscale, s_);
        for (int k = 0; k < D.ndca; ++k) fwn_gemm_launch(&D.dca[k], s_);
    }
    void wg_place(Deferred& D, float*& part) {          // split count of the block, partial regions of this flow's jobs
        TnList& tn = D.tn;
        TnSpec sp[4 + 5 * FWN_MAX_LAYERS];
        for (int k = 0; k < tn.n; ++k) sp[k] = {tn.job[k].Kx, tn.job[k].N, tn.job[k].ntap};
        const int ns = tn_block_splits(sp, tn.n, NF, (int)D.m);
        for (int k = 0; k < tn.n; ++k) {
            fwn_tn_job& q = tn.job[k];
            const long size = ((long)q.ntap * q.Kx + 1) * q.N;
            q.part = part; q.split_stride = size; q.nsplit = ns;
            part += (size_t)ns * size;
        }
    }
    int wg_wn(Deferred& D, hipStream_t s_) {
        TnList& tn = D.tn;
        for (int w0 = 0; w0 < D.nwn; w0 += FWN_MAX_GROUP) {
            const int cnt = D.nwn - w0 < FWN_MAX_GROUP ? D.nwn - w0 : FWN_MAX_GROUP;
            fwn_wn_job jobs[FWN_MAX_GROUP];
            for (int k = 0; k < cnt; ++k) {
                const WnItem& it = D.wn[w0 + k];
                fwn_wn_job& q = jobs[k];
                memset(&q, 0, sizeof(q));
                if (it.tn >= 0) {
                    const fwn_tn_job& tj = tn.job[it.tn];
                    q.part = tj.part; q.split_stride = tj.split_stride; q.nsplit = tj.nsplit; q.ldp = tj.N;
                    q.bias_row = tj.ntap * tj.Kx;
                } else {
                    q.part = it.part_direct; q.split_stride = it.part_stride; q.nsplit = it.part_nsplit; q.ldp = it.part_ld;
                    q.bias_row = it.part_rows - 1;
                }
                q.row_src = it.row_src; q.col_src = it.col_src; q.col0 = it.col0; q.K = it.k; q.N = it.n; q.scale = it.scale;
                q.V = it.c->g ? it.c->V : nullptr; q.g = it.c->g; q.dV = it.c->dV; q.dg = it.c->g ? it.c->dg : nullptr; q.db = it.c->db;
                TREQUIRE(q.dV && (!q.g || (q.V && q.dg)), "fwn_train_loss_and_grads: block %d: missing gradient / master pointer", D.i);
            }
            fwn_wn_group_launch(jobs, cnt, pl.wn_scratch, s_);
        }
        return FWN_OK;
    }
    int weight_grads(Deferred& D, hipStream_t s_) {        // one flow, start to end (the one-stream path)
        wg_small(D, s_);
        float* part = pl.tn_part;
        wg_place(D, part);
        for (int g0 = 0; g0 < D.tn.n; g0 += FWN_MAX_GROUP)
            fwn_tn_group_launch(D.tn.job + g0, D.tn.n - g0 < FWN_MAX_GROUP ? D.tn.n - g0 : FWN_MAX_GROUP, (int)D.m, (int)D.ti, s_);
        return wg_wn(D, s_);
    }
    // all flows of a block (side stream).  after_small: recorded on s_ behind stage (1) of the block's last flow (block 0: the
    // conditioning gradient is complete there)
    int weight_grads_block(std::vector<Deferred>& flows, hipStream_t s_, hipEvent_t after_small) {
        if (flows.empty()) return FWN_OK;
        const fwn_tn_job* gj[FWN_MAX_GROUP * 2];
        int gn[FWN_MAX_GROUP * 2], ng = 0;
        bool fits = true;
        for (size_t k = 0; k < flows.size(); ++k) ng += (flows[k].tn.n + FWN_MAX_GROUP - 1) / FWN_MAX_GROUP;
        if (ng > fwn_tn_multi_max() || ng > (int)(sizeof(gn) / sizeof(gn[0]))) fits = false;
        float* part = pl.tn_part;
        for (size_t k = 0; k < flows.size(); ++k) {
            wg_small(flows[k], s_);
            wg_place(flows[k], part);
        }
        if (after_small && hipEventRecord(after_small, s_) != hipSuccess)
            return fwn_set_error(FWN_ERR_HIP, "fwn_train_loss_and_grads: hipEventRecord failed");
        TREQUIRE(part - pl.tn_part <= tn_partial_floats(md, flows[0].i, flows[0].m),
                 "fwn_train_loss_and_grads: block %d: weight-gradient partials need %ld floats, planned %ld", flows[0].i,
                 (long)(part - pl.tn_part), tn_partial_floats(md, flows[0].i, flows[0].m));
        if (fits) {
            ng = 0;
            for (size_t k = 0; k < flows.size(); ++k)
                for (int g0 = 0; g0 < flows[k].tn.n; g0 += FWN_MAX_GROUP) {
                    gj[ng] = flows[k].tn.job + g0;
                    gn[ng++] = flows[k].tn.n - g0 < FWN_MAX_GROUP ? flows[k].tn.n - g0 : FWN_MAX_GROUP;
                }
            fwn_tn_multi_launch(gj, gn, ng, (int)flows[0].m, (int)flows[0].ti, pl.tn_table, s_);
        } else {
            for (size_t k = 0; k < flows.size(); ++k)
                for (int g0 = 0; g0 < flows[k].tn.n; g0 += FWN_MAX_GROUP)
                    fwn_tn_group_launch(flows[k].tn.job + g0, flows[k].tn.n - g0 < FWN_MAX_GROUP ? flows[k].tn.n - g0 : FWN_MAX_GROUP,
                                        (int)flows[k].m, (int)flows[k].ti, s_);
        }
        for (size_t k = 0; k < flows.size(); ++k) {
            const int rc = wg_wn(flows[k], s_);
            if (rc != FWN_OK) return rc;
        }
        return FWN_OK;
    }

    // ---- the side-stream protocol ----
    // everything enqueued on `st` so far happens before what `side` gets next
    bool fork_side() {
        hipEvent_t e = evp->get();
        forked = true;
        return e && hipEventRecord(e, st) == hipSuccess && hipStreamWaitEvent(side, e, 0) == hipSuccess;
    }
    bool join_side() {
        hipEvent_t e = evp->get();
        return e && hipEventRecord(e, side) == hipSuccess && hipStreamWaitEvent(st, e, 0) == hipSuccess;
    }
    bool join_pending() {      // the block handed over last: join it into `st`, then report it
        if (pending_block < 0) return true;
        if (!join_side()) return false;
        if (on_block_done && on_block_done(user, pending_block) != 0) hook_failed = true;
        pending_block = -1;
        return true;
    }
    int hand_over(bool last_block) {          // fork, then everything in `pending` to the side stream
        if (!fork_side()) return fwn_set_error(FWN_ERR_HIP, "fwn_train_loss_and_grads: forking the side stream failed");
        if (last_block) {
            dca_done = evp->get();
            if (!dca_done) return fwn_set_error(FWN_ERR_HIP, "fwn_train_loss_and_grads: hipEventCreate failed");
        }
        const int rc = weight_grads_block(pending, side, dca_done);
        if (rc != FWN_OK) return rc;
        pending.clear();
        return FWN_OK;
    }

    // ---------------- up-sampling transposed convolutions (model.py:301-311), last stage first ----------------
    int upsample_backward() {
        hipLaunchKernelGGL(planes_to_rows_kernel, dim3(grid_of(B * T * nmel)), dim3(256), 0, st, pl.dcplanes, (const bf16*)pl.cplanes, B * T, half, pl.up_dy,
                           pl.up_y);
        float* dy = pl.up_dy;
        const float* y = pl.up_y;
        for (int n = md->n_up - 1; n >= 0; --n) {
            const int s_ = md->up_scale[n];
            long hh = T / hop_of(md);
            for (int k = 0; k < n; ++k) hh *= md->up_scale[k];                 // rows of the stage's input
            const float* xin = n == 0 ? (len ? pl.melc : mel) : pl.ups[n - 1];      // ragged: the masked buffers of the forward half
            float* dx = n > 0 ? pl.up_dx[n & 1] : nullptr;
            const fwn_conv_grad& c = t->up[n];
            TREQUIRE(c.V && c.g && c.dV && c.dg && c.db, "fwn_train_loss_and_grads: up-sampling stage %d: missing pointer", n);
            fwn_up_bwd_launch(dy, y, xin, (int)B, (int)hh, nmel, s_, md->up_w[n], dx, pl.up_dwb, pl.up_scr, st);
            // ragged: the forward zeroed this stage's input past each clip's end - its gradient is dropped there before the
            // stage below reads it
            if (dx) rows.zero(dx, hh, (long)nmel * 4, (int)(T / hh));
            hipLaunchKernelGGL(up_prepare_kernel, dim3(1), dim3(64), 0, st, c.g, pl.up_g3);
            fwn_wn_job q;
            memset(&q, 0, sizeof(q));
            q.part = pl.up_dwb; q.split_stride = 0; q.nsplit = 1; q.ldp = 3; q.col0 = 0; q.bias_row = -1; q.K = 2 * s_; q.N = 3; q.scale = 1.0f;
            q.V = c.V; q.g = pl.up_g3; q.dV = c.dV; q.dg = pl.up_dg3; q.db = nullptr;
            fwn_wn_group_launch(&q, 1, pl.up_wn, st);
            hipLaunchKernelGGL(up_finish_kernel, dim3(1), dim3(64), 0, st, pl.up_dg3, pl.up_dwb, s_, c.dg, c.db);
            dy = dx;
            y = xin;
        }
        return FWN_OK;
    }
};

int train_call(PassKind kind, const fwn_train_desc* t, int64_t B, int64_t T, const float* x, const float* mel, const int32_t* len, void* workspace,
               size_t workspace_bytes, float* out3, float* out2B, fwn_block_done_fn on_block_done, void* user, void* stream) {
    TrainCall c;
    c.kind = kind; c.t = t; c.B = (long)B; c.T = (long)T; c.x = x; c.mel = mel; c.len = len;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.out3 = out3; c.out2B = out2B;
    c.on_block_done = on_block_done; c.user = user; c.st = (hipStream_t)stream;
    return c.run();
}

}  // namespace

extern "C" {

size_t fwn_train_workspace_bytes(const fwn_train_desc* t, int64_t B, int64_t T) { return train_workspace(t, B, T, PASS_TRAIN); }
size_t fwn_train_ragged_workspace_bytes(const fwn_train_desc* t, int64_t B, int64_t T) {
    if (B >= 32768 || (t && t->model && t->model->gate_fp8)) return 0;
    return train_workspace(t, B, T, PASS_TRAIN_RAGGED);
}
int fwn_train_loss_and_grads(const fwn_train_desc* t, int64_t B, int64_t T, const float* x, const float* mel, void* workspace,
                             size_t workspace_bytes, float* out3, fwn_block_done_fn on_block_done, void* user, void* stream) {
    return train_call(PASS_TRAIN, t, B, T, x, mel, nullptr, workspace, workspace_bytes, out3, nullptr, on_block_done, user, stream);
}
int fwn_train_loss_and_grads_ragged(const fwn_train_desc* t, int64_t B, int64_t T, const float* x, const float* mel, const int32_t* len_dev,
                                    void* workspace, size_t workspace_bytes, float* out3, float* out2B, fwn_block_done_fn on_block_done,
                                    void* user, void* stream) {
    TREQUIRE(len_dev, "fwn_train_loss_and_grads_ragged: null lengths");
    return train_call(PASS_TRAIN_RAGGED, t, B, T, x, mel, len_dev, workspace, workspace_bytes, out3, out2B, on_block_done, user, stream);
}

}  // extern "C"
