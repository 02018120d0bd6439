// C-ABI of libfwn.so (declared in include/fwn.h): argument validation, workspace carving and
// launch sequencing for the flow forward / inverse path.  No allocation, no synchronisation.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <initializer_list>

#include "../../include/fwn.h"
#include "fwn_internal.h"
#include "fwn_sequence.h"

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
// the same for the other translation units of the library (train_api.hip)
int fwn_set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
static int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FWN_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return FWN_OK;
}
#define REQUIRE(cond, ...) do { if (!(cond)) return fail(FWN_ERR_ARG, __VA_ARGS__); } while (0)
#define ALIGNED16(p) ((((uintptr_t)(p)) & 15) == 0)
#define ALIGNED8(p) ((((uintptr_t)(p)) & 7) == 0)
#define ALIGNED4(p) ((((uintptr_t)(p)) & 3) == 0)

// ---- the hoisted conditioning of one block (inference and training; each has its own hoisting rule) ----
fwn_cond_plan fwn_plan_cond(bool hoist, int M, int nflow, int L, int cin, int kcpad, const void* stream) {
    fwn_cond_plan cp{hoist, nullptr, false, 1};
    if (!hoist) return cp;
    if (fwn_cond_rs_wanted(M, cin, kcpad, nflow * L, stream != nullptr)) {
        cp.stream = stream;
        cp.nsplit = fwn_cond_rs_nsplit(M, nflow * L, kcpad);
    } else {
        const int nzg = ((nflow + 1) / 2) * L;
        cp.nsplit = fwn_cond_nsplit(M, nzg, kcpad);
        cp.merged = nflow > 1 && fwn_cond_merge(M, nzg, cp.nsplit);
    }
    return cp;
}
void fwn_run_cond(const fwn_cond_plan& cp, const void* ca0, const void* ca1, const void* Wc0, float* P, float* Ppart, int M, int nflow,
                  int L, int cin, int kcpad, hipStream_t st) {
    const long pn = (long)nflow * L * M * 512;          // floats of the block's P matrices
    if (cp.stream)          // the block's matrices from their fragment streams (csrc/cond_rs.h)
        fwn_launch_cond_rs(ca0, nflow > 1 ? ca1 : nullptr, cp.stream, P, nflow * L, L, M, cin, kcpad, Ppart, pn, cp.nsplit, st);
    else if (cp.merged)
        fwn_launch_cond2(ca0, ca1, Wc0, P, (long)512 * kcpad, (long)M * 512, 0, 1, nflow, L, M, cin, kcpad, Ppart, pn, cp.nsplit, st);
    else
        for (int g = 0; g < 2 && g < nflow; ++g)
            fwn_launch_cond(g ? ca1 : ca0, Wc0, P, (long)512 * kcpad, (long)M * 512, g, 2, (nflow - g + 1) / 2, L, M, cin, kcpad, Ppart,
                            pn, cp.nsplit, st);
    fwn_launch_cond_reduce(P, Ppart, pn, cp.nsplit, pn, st);
}

// ---- the ragged forward rules and the two stage walks of both sequencers (fwn_sequence.h) ----
void ClipRows::zero(void* base, long rows, long row_bytes, int samples_per_row) const {
    if (len) fwn_launch_mask_rows(base, B, rows, row_bytes, len, (int)B, samples_per_row, st);
}
void ClipRows::zero_planes(float* planes, long T) const { if (len) fwn_launch_mask_rows(planes, 2 * B, T / 2, 4, len, (int)B, 2, st); }
void ClipRows::neg_shift(float* xa, long rows, int Ch, const float* shift) const {
    if (len) fwn_launch_fill_neg_shift(xa, B, rows, Ch, shift, len, (int)B, 2 * Ch, st);
}

int fwn_run_upsample(const fwn_model_desc* m, long B, long T, const float* mel, const UpsampleBufs& u, const ClipRows& rows) {
    const int nmel = 2 * (m->num_mels / 2);
    int H = (int)(T / hop_of(m));
    int spr = hop_of(m);                 // samples per row of the current stage's input
    const float* in = mel;
    if (rows.len) {
        if (hipMemcpyAsync(u.mel_copy, mel, (size_t)B * H * nmel * 4, hipMemcpyDeviceToDevice, rows.st) != hipSuccess) return -1;
        rows.zero(u.mel_copy, H, (long)nmel * 4, spr);
        in = u.mel_copy;
    }
    for (int i = 0; i < m->n_up; ++i) {
        const bool last = (i == m->n_up - 1);
        float* outf = last ? nullptr : u.inner[i];
        fwn_launch_upsample(in, (int)B, H, nmel, m->up_w[i], u.bias_dev ? 0.0f : m->up_bias[i], u.bias_dev ? u.bias_dev[i] : nullptr,
                            m->up_scale[i], outf, last ? u.cplanes : nullptr, rows.st);
        H *= m->up_scale[i];
        spr /= m->up_scale[i];
        if (!last) rows.zero(outf, H, (long)nmel * 4, spr);
        in = outf;
    }
    return 0;
}

void fwn_run_stages(const fwn_flow_desc* d, const FlowStages& s, float* xa, const void* ca, const float* P, int M, int Ti, int inverse,
                    const ClipRows& rows) {
    hipStream_t st = rows.st;
    // h rows past a clip's end are zeroed behind every kernel that writes h, so that the taps of the next one read what they
    // read at the end of a clip on its own - and BEFORE h is kept (training's weight gradients read it)
    if (!inverse) rows.neg_shift(xa, Ti, d->Ch, d->an);
    if (!s.have_h0)
        fwn_launch_front(xa, d->an, d->Wfront, d->Wfront2, d->bfront, s.h[0], s.front_scratch, M, Ti, d->Ch, d->kfpad, inverse ? 0 : 1,
                         s.h8[0], st);
    rows.zero(s.h[0], Ti, 512, 2 * d->Ch);
    for (int l = 0; l < d->L; ++l) {
        if (s.h8[l])
            fwn_launch_gate_fp8(s.h8[l], ca, d->Wd8[l], d->wd8_exp[l], d->Wc[l], d->bgate[l], s.o[l], M, Ti, dilation_of(l), d->cin,
                                d->kcpad, st);
        else
            fwn_launch_gate(s.h[l], ca, P ? P + (size_t)l * M * 512 : nullptr, d->Wd[l], d->Wc[l], s.gate_stream ? d->Wgs[l] : nullptr,
                            s.gate_stream ? d->Wds[l] : nullptr, d->bgate[l], s.o[l], M, Ti, dilation_of(l), d->cin, d->kcpad, s.aux[l], st);
        if (l + 1 < d->L) {
            fwn_launch_res(s.o[l], s.h[l], d->Wres[l], d->bres[l], s.h[l + 1], M, s.h8[l + 1], st);
            rows.zero(s.h[l + 1], Ti, 512, 2 * d->Ch);
        }
    }
}

extern "C" {

int fwn_version(void) { return FWN_VERSION; }
const char* fwn_last_error(void) { return g_err; }

int fwn_wn_scale(const float* v, const float* g, int k_src, int n_src, float* scale, void* stream) {
    REQUIRE(v && g && scale, "fwn_wn_scale: null pointer");
    REQUIRE(k_src > 0 && n_src > 0, "fwn_wn_scale: bad shape %d x %d", k_src, n_src);
    fwn_launch_wn_scale(v, g, k_src, n_src, scale, (hipStream_t)stream);
    return check_launch("fwn_wn_scale");
}

int fwn_pack_bf16(const float* v, const float* scale, const int32_t* src_k, const int32_t* src_n,
                  int n_src, int k_dst, int n_dst, int64_t ld_dst, void* out_bf16, void* stream) {
    REQUIRE(v && src_k && src_n && out_bf16, "fwn_pack_bf16: null pointer");
    REQUIRE(n_src > 0 && k_dst > 0 && n_dst > 0 && ld_dst >= k_dst, "fwn_pack_bf16: bad shape");
    fwn_launch_pack(v, scale, src_k, src_n, n_src, k_dst, n_dst, (long)ld_dst, out_bf16, (hipStream_t)stream);
    return check_launch("fwn_pack_bf16");
}

int fwn_pack_jobs(const fwn_scale_job* scale_jobs, int n_scale_jobs, const fwn_pack_job* pack_jobs, int n_pack_jobs,
                  float* scales, int scale_ld, void* stream) {
    REQUIRE(n_scale_jobs >= 0 && n_pack_jobs >= 0 && (n_scale_jobs == 0 || (scale_jobs && scales)) &&
                (n_pack_jobs == 0 || pack_jobs) && scale_ld > 0 && scale_ld % 32 == 0, "fwn_pack_jobs: bad argument");
    REQUIRE(n_scale_jobs < 65536 * 32 && n_pack_jobs < 65536, "fwn_pack_jobs: too many jobs (the pack job index is gridDim.y)");
    fwn_launch_pack_jobs(scale_jobs, n_scale_jobs, pack_jobs, n_pack_jobs, scales, scale_ld, (hipStream_t)stream);
    return check_launch("fwn_pack_jobs");
}

int fwn_gather_tables(const float* flat, const int64_t* idx, int nterm, int64_t total, const double* post,
                      const unsigned char* mode, float* out, void* stream) {
    REQUIRE(flat && idx && post && mode && out && nterm >= 1 && total > 0, "fwn_gather_tables: bad argument");
    fwn_launch_gather_tables(flat, (const long long*)idx, nterm, (long)total, post, mode, out, (hipStream_t)stream);
    return check_launch("fwn_gather_tables");
}
int fwn_sum_f32(const float* in, int64_t n, float* out, void* stream) {
    REQUIRE(in && out && n > 0, "fwn_sum_f32: bad argument");
    fwn_launch_sum_f32(in, (long)n, out, (hipStream_t)stream);
    return check_launch("fwn_sum_f32");
}
int fwn_upsample_wn(const float* v, const float* g, int s, float* out, void* stream) {
    REQUIRE(v && g && out && s > 0, "fwn_upsample_wn: bad argument");
    fwn_launch_upsample_wn(v, g, s, out, (hipStream_t)stream);
    return check_launch("fwn_upsample_wn");
}

int fwn_upsample_stage(const float* in, int B, int H, int W, const float* wk, float bias, int s,
                       float* out_f32, void* out_cplanes, void* stream) {
    REQUIRE(in && wk, "fwn_upsample_stage: null pointer");
    REQUIRE((out_f32 != nullptr) != (out_cplanes != nullptr), "fwn_upsample_stage: exactly one output");
    REQUIRE(B > 0 && H > 0 && W > 0 && s > 0 && (s % 2) == 0, "fwn_upsample_stage: bad shape (s must be even)");
    REQUIRE(!out_cplanes || (W % 2) == 0, "fwn_upsample_stage: W must be even for planes");
    fwn_launch_upsample(in, B, H, W, wk, bias, nullptr, s, out_f32, out_cplanes, (hipStream_t)stream);
    return check_launch("fwn_upsample_stage");
}
int fwn_upsample_stage_dev(const float* in, int B, int H, int W, const float* wk, const float* bias, int s,
                           float* out_f32, void* out_cplanes, void* stream) {
    REQUIRE(in && wk && bias, "fwn_upsample_stage_dev: null pointer");
    REQUIRE((out_f32 != nullptr) != (out_cplanes != nullptr), "fwn_upsample_stage_dev: exactly one output");
    REQUIRE(B > 0 && H > 0 && W > 0 && s > 0 && (s % 2) == 0, "fwn_upsample_stage_dev: bad shape (s must be even)");
    REQUIRE(!out_cplanes || (W % 2) == 0, "fwn_upsample_stage_dev: W must be even for planes");
    fwn_launch_upsample(in, B, H, W, wk, 0.0f, bias, s, out_f32, out_cplanes, (hipStream_t)stream);
    return check_launch("fwn_upsample_stage_dev");
}

int fwn_split_planes(const float* x, int64_t B, int64_t T, float* planes, void* stream) {
    REQUIRE(x && planes && B > 0 && T > 0 && (T % 2) == 0, "fwn_split_planes: bad argument");
    fwn_launch_split(x, B, T, planes, (hipStream_t)stream);
    return check_launch("fwn_split_planes");
}
int fwn_merge_planes(const float* planes, int64_t B, int64_t T, float* x, void* stream) {
    REQUIRE(x && planes && B > 0 && T > 0 && (T % 2) == 0, "fwn_merge_planes: bad argument");
    fwn_launch_merge(planes, B, T, x, (hipStream_t)stream);
    return check_launch("fwn_merge_planes");
}
int fwn_mask_rows(void* base, int64_t B, int64_t rows, int64_t row_bytes, const int32_t* len, int32_t samples_per_row, void* stream) {
    REQUIRE(base && len && B > 0 && B < 65536 && rows > 0 && row_bytes > 0 && samples_per_row > 0, "fwn_mask_rows: bad argument");
    REQUIRE((((uintptr_t)base) & 3) == 0 && row_bytes % 4 == 0, "fwn_mask_rows: base and row_bytes must be multiples of 4");
    REQUIRE(rows <= ((int64_t)1 << 31) / samples_per_row, "fwn_mask_rows: rows * samples_per_row exceeds 2^31");
    fwn_launch_mask_rows(base, (long)B, (long)rows, (long)row_bytes, len, (int)B, samples_per_row, (hipStream_t)stream);
    return check_launch("fwn_mask_rows");
}

int fwn_fill_neg_shift(float* plane, int64_t B, int64_t rows, int Ch, const float* shift, const int32_t* len,
                       int32_t samples_per_row, void* stream) {
    REQUIRE(plane && shift && len && B > 0 && B < 65536 && rows > 0 && samples_per_row > 0, "fwn_fill_neg_shift: bad argument");
    REQUIRE(Ch >= 1 && (Ch & (Ch - 1)) == 0, "fwn_fill_neg_shift: Ch=%d must be a power of two", Ch);
    REQUIRE((((uintptr_t)plane) & 3) == 0, "fwn_fill_neg_shift: plane must be 4-byte aligned");
    REQUIRE(rows <= ((int64_t)1 << 31) / samples_per_row, "fwn_fill_neg_shift: rows * samples_per_row exceeds 2^31");
    fwn_launch_fill_neg_shift(plane, (long)B, (long)rows, Ch, shift, len, (int)B, samples_per_row, (hipStream_t)stream);
    return check_launch("fwn_fill_neg_shift");
}
int fwn_ragged_logdet_slots(int64_t B) { return B > 0 ? fwn_ragged_logdet_nslot((long)B) : 0; }
int fwn_ragged_logdet_rows(const float* Z, int64_t B, int64_t rows, int Ch, const float* ez, const float* an, const int32_t* len,
                           int32_t samples_per_row, double* acc, void* stream) {
    REQUIRE(Z && ez && len && acc && B > 0 && B < 65536 && rows > 0 && samples_per_row > 0, "fwn_ragged_logdet_rows: bad argument");
    REQUIRE(Ch >= 1 && (Ch & (Ch - 1)) == 0, "fwn_ragged_logdet_rows: Ch=%d must be a power of two", Ch);
    REQUIRE(ALIGNED4(Z) && ALIGNED8(acc), "fwn_ragged_logdet_rows: misaligned buffer");
    REQUIRE(rows <= ((int64_t)1 << 31) / samples_per_row, "fwn_ragged_logdet_rows: rows * samples_per_row exceeds 2^31");
    fwn_launch_range_logdet(Z, (long)B, (long)rows, Ch, ez, an, nullptr, len, (int)B, samples_per_row, acc, (hipStream_t)stream);
    return check_launch("fwn_ragged_logdet_rows");
}

int fwn_actnorm_ddi(const float* xa, const float* xb, int M, int Ch, float* an, void* stream) {
    REQUIRE(xa && xb && an && M > 0 && Ch > 0, "fwn_actnorm_ddi: bad argument");
    fwn_launch_ddi(xa, xb, M, Ch, an, (hipStream_t)stream);
    return check_launch("fwn_actnorm_ddi");
}

int fwn_actnorm_moments(const float* xa, const float* xb, int M, int Ch, double* mom, void* stream) {
    REQUIRE(xa && xb && mom && M > 0 && Ch > 0, "fwn_actnorm_moments: bad argument");
    fwn_launch_ddi_moments(xa, xb, M, Ch, mom, (hipStream_t)stream);
    return check_launch("fwn_actnorm_moments");
}
int fwn_actnorm_from_moments(const double* mom, int Ch, float* an, void* stream) {
    REQUIRE(mom && an && Ch > 0, "fwn_actnorm_from_moments: bad argument");
    fwn_launch_ddi_from_moments(mom, Ch, an, (hipStream_t)stream);
    return check_launch("fwn_actnorm_from_moments");
}

int64_t fwn_actnorm_moments_ragged_scratch_bytes(int64_t B, int64_t rows, int Ch) {
    if (B <= 0 || B >= 65536 || rows <= 0 || Ch < 1 || (Ch & (Ch - 1)) != 0 || B * rows > ((int64_t)1 << 40) / Ch) return 0;
    return (int64_t)fwn_ragged_moments_nslot((long)B, (long)rows, Ch) * 4 * Ch * 8;
}
int fwn_actnorm_moments_ragged(const float* xa, const float* xb, int64_t B, int64_t rows, int Ch, const int32_t* len,
                               int32_t samples_per_row, double* mom, double* scratch, int64_t scratch_bytes, void* stream) {
    REQUIRE(xa && xb && len && mom && scratch && B > 0 && B < 65536 && rows > 0 && samples_per_row > 0, "fwn_actnorm_moments_ragged: bad argument");
    REQUIRE(Ch >= 1 && (Ch & (Ch - 1)) == 0, "fwn_actnorm_moments_ragged: Ch=%d must be a power of two", Ch);
    REQUIRE(((((uintptr_t)xa) | ((uintptr_t)xb)) & 3) == 0 && ((((uintptr_t)mom) | ((uintptr_t)scratch)) & 7) == 0,
            "fwn_actnorm_moments_ragged: misaligned buffer");
    REQUIRE(rows <= ((int64_t)1 << 31) / samples_per_row && B * rows <= ((int64_t)1 << 40) / Ch, "fwn_actnorm_moments_ragged: shape too large");
    const int64_t need = fwn_actnorm_moments_ragged_scratch_bytes(B, rows, Ch);
    REQUIRE(scratch_bytes >= need, "fwn_actnorm_moments_ragged: scratch of %lld bytes, %lld needed (fwn_actnorm_moments_ragged_scratch_bytes)",
            (long long)scratch_bytes, (long long)need);
    fwn_launch_ddi_moments_ragged(xa, xb, (long)B, (long)rows, Ch, len, samples_per_row, mom, scratch, (hipStream_t)stream);
    return check_launch("fwn_actnorm_moments_ragged");
}

static int check_desc(const fwn_flow_desc* d) {
    REQUIRE(d, "flow desc is null");
    REQUIRE(d->Ch >= 1 && (d->Ch & (d->Ch - 1)) == 0, "flow desc: Ch=%d must be a power of two", d->Ch);
    REQUIRE(d->L >= 1 && d->L <= FWN_MAX_LAYERS, "flow desc: L=%d out of range", d->L);
    REQUIRE(d->cin > 0 && d->cin % 8 == 0, "flow desc: cin=%d must be a multiple of 8", d->cin);
    REQUIRE(d->kcpad % 64 == 0 && d->kcpad >= d->cin, "flow desc: kcpad=%d", d->kcpad);
    REQUIRE(d->kfpad % 64 == 0 && d->kfpad >= 3 * d->Ch, "flow desc: kfpad=%d", d->kfpad);
    REQUIRE(d->npt >= 1 && d->npt * 32 >= d->Ch, "flow desc: npt=%d", d->npt);
    REQUIRE(d->Wfront && d->bfront && d->Wskip && d->bskip && d->Wfinal && d->bfinal && d->Wzero &&
            d->bzero && d->ezero && d->an, "flow desc: null weight pointer");
    for (int l = 0; l < d->L; ++l) {
        REQUIRE(d->Wd[l] && d->Wc[l] && d->bgate[l], "flow desc: null gate weights (layer %d)", l);
        REQUIRE(l == d->L - 1 || (d->Wres[l] && d->bres[l]), "flow desc: null res weights (layer %d)", l);
        REQUIRE(ALIGNED16(d->Wd[l]) && ALIGNED16(d->Wc[l]), "flow desc: weights must be 16-byte aligned");
    }
    REQUIRE(ALIGNED16(d->Wfront) && ALIGNED16(d->Wskip) && ALIGNED16(d->Wfinal) && ALIGNED16(d->Wzero),
            "flow desc: weights must be 16-byte aligned");
    for (int l = 0; l < d->L; ++l)
        REQUIRE(!d->Wgs[l] || (ALIGNED16(d->Wgs[l]) && fwn_gate_stream_size(d->cin) != 0),
                "flow desc: Wgs[%d] given but no register-streamed gate kernel exists for cin = %d (or misaligned)", l, d->cin);
    REQUIRE(!d->Wts || (ALIGNED16(d->Wts) && fwn_tail_stream_size(d->L) != 0),
            "flow desc: Wts given but no register-streamed tail kernel exists for L = %d (or misaligned)", d->L);
    for (int l = 0; l < d->L; ++l) REQUIRE(!d->Wds[l] || ALIGNED16(d->Wds[l]), "flow desc: Wds[%d] misaligned", l);
    if (d->Wfront3)
        REQUIRE(d->Ch <= 8 && d->kf3 == (6 * d->Ch + 15) / 16 * 16 && ALIGNED16(d->Wfront3),
                "flow desc: Wfront3 needs Ch <= 8 and kf3 = 6 Ch rounded up to 16 (Ch %d, kf3 %d)", d->Ch, d->kf3);
    return FWN_OK;
}

int fwn_front(const fwn_flow_desc* d, const float* xa, void* h_out, void* scratch, int M, int Ti, int apply_an,
              void* stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    REQUIRE(xa && h_out && M > 0 && Ti > 0 && M % Ti == 0, "fwn_front: bad argument");
    REQUIRE(ALIGNED16(xa) && ALIGNED16(h_out), "fwn_front: buffers must be 16-byte aligned");
    REQUIRE(!scratch || ALIGNED16(scratch), "fwn_front: scratch must be 16-byte aligned");
    fwn_launch_front(xa, d->an, d->Wfront, d->Wfront2, d->bfront, h_out, scratch, M, Ti, d->Ch, d->kfpad, apply_an,
                     nullptr, (hipStream_t)stream);
    return check_launch("fwn_front");
}

int fwn_gate(const fwn_flow_desc* d, int layer, const void* h, const void* ca, const float* P, void* o,
             int M, int Ti, void* stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    REQUIRE(layer >= 0 && layer < d->L, "fwn_gate: layer %d out of range", layer);
    REQUIRE(h && o && M > 0 && Ti > 0 && M % Ti == 0, "fwn_gate: bad argument");
    REQUIRE((ca != nullptr) != (P != nullptr), "fwn_gate: exactly one of ca / P");
    REQUIRE(ALIGNED16(h) && ALIGNED16(o) && ALIGNED16(ca), "fwn_gate: buffers must be 16-byte aligned");
    fwn_launch_gate(h, ca, P, d->Wd[layer], d->Wc[layer], d->Wgs[layer], d->Wds[layer], d->bgate[layer], o, M, Ti,
                    dilation_of(layer), d->cin, d->kcpad, nullptr, (hipStream_t)stream);
    return check_launch("fwn_gate");
}

int fwn_gate_tile(const fwn_flow_desc* d, int layer, const void* h, const float* P, void* o, int M, int Ti, int rows, int cols,
                  void* stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    REQUIRE(layer >= 0 && layer < d->L && h && P && o && M > 0 && Ti > 0 && M % Ti == 0, "fwn_gate_tile: bad argument");
    REQUIRE(ALIGNED16(h) && ALIGNED16(o), "fwn_gate_tile: buffers must be 16-byte aligned");
    int n = 0;
    if (cols == 128) {
        n = fwn_launch_gate_ring_tile(h, P, d->Wd[layer], d->bgate[layer], o, M, Ti, dilation_of(layer), rows, (hipStream_t)stream);
    } else {
        REQUIRE(d->Wds[layer], "fwn_gate_tile: the flow has no Wd stream (fwn_flow_desc.Wds)");
        REQUIRE(fwn_gate_hs_ok(M, Ti, dilation_of(layer)), "fwn_gate_tile: M = %d, Ti = %d, layer %d is outside the streamed hoisted gate's range", M, Ti, layer);
        n = fwn_launch_gate_hs(h, d->Wds[layer], d->bgate[layer], P, o, M, Ti, dilation_of(layer), rows, cols, (hipStream_t)stream);
    }
    REQUIRE(n > 0, "fwn_gate_tile: no %d x %d tile", rows, cols);
    rc = check_launch("fwn_gate_tile");
    return rc ? rc : n;
}

int fwn_gate_train(const fwn_flow_desc* d, int layer, const void* h, const void* ca, const float* P, void* o, void* aux,
                   int M, int Ti, void* stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    REQUIRE(layer >= 0 && layer < d->L, "fwn_gate_train: layer %d out of range", layer);
    REQUIRE(h && o && aux && M > 0 && Ti > 0 && M % Ti == 0, "fwn_gate_train: bad argument");
    REQUIRE((ca != nullptr) != (P != nullptr), "fwn_gate_train: exactly one of ca / P");
    REQUIRE(ALIGNED16(h) && (!ca || ALIGNED16(ca)), "fwn_gate_train: buffers must be 16-byte aligned");
    fwn_launch_gate(h, ca, P, d->Wd[layer], d->Wc[layer], nullptr, nullptr, d->bgate[layer], o, M, Ti, dilation_of(layer),
                    d->cin, d->kcpad, aux, (hipStream_t)stream);
    return check_launch("fwn_gate_train");
}

int fwn_gate_clock(const fwn_flow_desc* d, int layer, const void* h, const void* ca, void* o, int M, int Ti, uint64_t* stamps,
                   void* stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    REQUIRE(layer >= 0 && layer < d->L && h && ca && o && stamps && M > 0 && Ti > 0 && M % Ti == 0, "fwn_gate_clock: bad argument");
    REQUIRE(ALIGNED16(h) && ALIGNED16(ca) && ALIGNED16(o) && (((uintptr_t)stamps) & 7) == 0, "fwn_gate_clock: misaligned buffer");
    const int n = fwn_launch_gate_clock(h, ca, d->Wgs[layer], d->bgate[layer], o, M, Ti, dilation_of(layer), d->cin,
                                        (unsigned long long*)stamps, (hipStream_t)stream);
    REQUIRE(n > 0, "fwn_gate_clock: no 256-row register-streamed gate for this shape (M = %d, cin = %d, Wgs %s)", M, d->cin,
            d->Wgs[layer] ? "set" : "NULL");
    rc = check_launch("fwn_gate_clock");
    return rc ? rc : n;
}

int64_t fwn_gate_stream_bytes(int cin) { return cin > 0 ? (int64_t)fwn_gate_stream_size(cin) : 0; }
int fwn_gate_stream_rows(void) { return fwn_gate_stream_min_rows(); }
int fwn_pack_gate_stream(const void* Wd, const void* Wc, int cin, int kcpad, void* out, void* stream) {
    REQUIRE(Wd && Wc && out && cin > 0 && kcpad >= cin && kcpad % 64 == 0, "fwn_pack_gate_stream: bad argument");
    REQUIRE(fwn_gate_stream_size(cin) != 0, "fwn_pack_gate_stream: no register-streamed gate kernel for cin = %d", cin);
    REQUIRE(ALIGNED16(Wd) && ALIGNED16(Wc) && ALIGNED16(out), "fwn_pack_gate_stream: buffers must be 16-byte aligned");
    fwn_launch_gate_stream_pack(Wd, Wc, cin, kcpad, out, (hipStream_t)stream);
    return check_launch("fwn_pack_gate_stream");
}

int fwn_gate_fp8_supported(int M, int layer) {
    return layer >= 0 && layer < FWN_MAX_LAYERS && M > 0 && fwn_gate_fp8_ok(M, dilation_of(layer)) ? 1 : 0;
}
int fwn_gate_fp8(const fwn_flow_desc* d, int layer, const void* h8, const void* ca, void* o, int M, int Ti, void* stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    REQUIRE(layer >= 0 && layer < d->L, "fwn_gate_fp8: layer %d out of range", layer);
    REQUIRE(h8 && ca && o && M > 0 && Ti > 0 && M % Ti == 0, "fwn_gate_fp8: bad argument");
    REQUIRE(d->Wd8[layer], "fwn_gate_fp8: the flow has no e4m3 weights (fwn_pack_e4m3)");
    REQUIRE(fwn_gate_fp8_supported(M, layer), "fwn_gate_fp8: no fp8 kernel for M=%d, layer %d (needs M >= 12288, dilation <= 3)", M, layer);
    REQUIRE(ALIGNED16(h8) && ALIGNED16(o) && ALIGNED16(ca) && ALIGNED16(d->Wd8[layer]), "fwn_gate_fp8: buffers must be 16-byte aligned");
    fwn_launch_gate_fp8(h8, ca, d->Wd8[layer], d->wd8_exp[layer], d->Wc[layer], d->bgate[layer], o, M, Ti, dilation_of(layer),
                        d->cin, d->kcpad, (hipStream_t)stream);
    return check_launch("fwn_gate_fp8");
}
int fwn_cast_e4m3(const void* src_bf16, void* dst_u8, int64_t n, void* stream) {
    REQUIRE(src_bf16 && dst_u8 && n > 0, "fwn_cast_e4m3: bad argument");
    fwn_launch_cast_e4m3(src_bf16, dst_u8, (long)n, (hipStream_t)stream);
    return check_launch("fwn_cast_e4m3");
}
int fwn_wn_absmax(const float* v, const float* scale, int k_src, int n_src, float mul, float* amax, void* stream) {
    REQUIRE(v && amax && k_src > 0 && n_src > 0, "fwn_wn_absmax: bad argument");
    fwn_launch_wn_absmax(v, scale, k_src, n_src, mul, amax, (hipStream_t)stream);
    return check_launch("fwn_wn_absmax");
}
int fwn_pack_e4m3(const float* v, const float* scale, const int32_t* src_k, const int32_t* src_n, int n_src, int k_dst,
                  int n_dst, int64_t ld_dst, float mul, const float* amax, void* out_u8, int32_t* exp_out, void* stream) {
    REQUIRE(v && src_k && src_n && amax && out_u8 && exp_out, "fwn_pack_e4m3: null pointer");
    REQUIRE(n_src > 0 && k_dst > 0 && n_dst > 0 && ld_dst >= k_dst, "fwn_pack_e4m3: bad shape");
    fwn_launch_pack_e4m3(v, scale, src_k, src_n, n_src, k_dst, n_dst, (long)ld_dst, mul, amax, out_u8, exp_out, (hipStream_t)stream);
    return check_launch("fwn_pack_e4m3");
}

int fwn_res(const fwn_flow_desc* d, int layer, const void* o, const void* h_in, void* h_out, int M,
            void* stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    REQUIRE(layer >= 0 && layer < d->L - 1, "fwn_res: layer %d has no live res_conv", layer);
    REQUIRE(o && h_in && h_out && M > 0, "fwn_res: bad argument");
    fwn_launch_res(o, h_in, d->Wres[layer], d->bres[layer], h_out, M, nullptr, (hipStream_t)stream);
    return check_launch("fwn_res");
}

int fwn_cond(const void* ca, const void* Wc_base, float* P_base, int64_t w_stride, int64_t p_stride,
             int flow0, int flow_step, int nflow, int L, int M, int cin, int kcpad, void* stream) {
    REQUIRE(ca && Wc_base && P_base, "fwn_cond: null pointer");
    REQUIRE(nflow > 0 && L > 0 && M > 0 && cin > 0 && cin % 8 == 0 && kcpad % 64 == 0 && kcpad >= cin,
            "fwn_cond: bad shape");
    REQUIRE(flow0 >= 0 && flow_step > 0, "fwn_cond: bad flow group");
    fwn_launch_cond(ca, Wc_base, P_base, (long)w_stride, (long)p_stride, flow0, flow_step, nflow, L, M, cin,
                    kcpad, nullptr, 0, 1, (hipStream_t)stream);
    return check_launch("fwn_cond");
}

int fwn_cond_splits(int M, int nz, int kcpad) { return (M > 0 && nz > 0 && kcpad > 0) ? fwn_cond_nsplit(M, nz, kcpad) : 1; }
int fwn_cond_split(const void* ca, const void* Wc_base, float* P_base, int64_t w_stride, int64_t p_stride,
                   int flow0, int flow_step, int nflow, int L, int M, int cin, int kcpad, float* part, int64_t part_stride,
                   int nsplit, void* stream) {
    REQUIRE(ca && Wc_base && P_base, "fwn_cond_split: null pointer");
    REQUIRE(nflow > 0 && L > 0 && M > 0 && cin > 0 && cin % 8 == 0 && kcpad % 64 == 0 && kcpad >= cin,
            "fwn_cond_split: bad shape");
    REQUIRE(flow0 >= 0 && flow_step > 0, "fwn_cond_split: bad flow group");
    REQUIRE(nsplit >= 1 && nsplit <= kcpad / 64 && (nsplit == 1 || (part && part_stride > 0 && part_stride % 4 == 0)),
            "fwn_cond_split: nsplit=%d needs a partial buffer and at most one split per 64-wide chunk", nsplit);
    fwn_launch_cond(ca, Wc_base, P_base, (long)w_stride, (long)p_stride, flow0, flow_step, nflow, L, M, cin,
                    kcpad, part, (long)part_stride, nsplit, (hipStream_t)stream);
    return check_launch("fwn_cond_split");
}
int fwn_cond_reduce(float* P, const float* part, int64_t part_stride, int nsplit, int64_t n, void* stream) {
    REQUIRE(P && n > 0 && n % 4 == 0 && nsplit >= 1 && (nsplit == 1 || (part && part_stride >= n)), "fwn_cond_reduce: bad argument");
    fwn_launch_cond_reduce(P, part, (long)part_stride, nsplit, (long)n, (hipStream_t)stream);
    return check_launch("fwn_cond_reduce");
}
int64_t fwn_cond_stream_bytes(int kcpad) { return (int64_t)fwn_cond_stream_size(kcpad); }
int fwn_cond_stream_rows(void) { return fwn_cond_stream_min_rows(); }
int fwn_cond_stream_splits(int M, int nz, int kcpad) { return (M > 0 && nz > 0 && kcpad >= 64) ? fwn_cond_rs_nsplit(M, nz, kcpad) : 1; }
int fwn_pack_cond_stream(const void* Wc_base, int64_t w_stride, int kcpad, int nz, void* out, void* stream) {
    REQUIRE(Wc_base && out && nz > 0 && fwn_cond_stream_size(kcpad) != 0 && w_stride >= (int64_t)512 * kcpad && w_stride % 8 == 0,
            "fwn_pack_cond_stream: bad argument");
    REQUIRE(((uintptr_t)Wc_base & 15) == 0 && ((uintptr_t)out & 15) == 0, "fwn_pack_cond_stream: 16-byte aligned operands");
    fwn_launch_cond_stream_pack(Wc_base, (long)w_stride, kcpad, nz, out, (hipStream_t)stream);
    return check_launch("fwn_pack_cond_stream");
}
int fwn_cond_stream(const void* ca, const void* ca_odd, const void* Ws, float* P, int nflow, int L, int M, int cin, int kcpad,
                    float* part, int64_t part_stride, int nsplit, void* stream) {
    REQUIRE(ca && Ws && P && nflow > 0 && L > 0, "fwn_cond_stream: null pointer / bad counts");
    REQUIRE(fwn_cond_rs_ok(M, cin, kcpad, true) && kcpad >= cin, "fwn_cond_stream: no register-streamed kernel for M=%d cin=%d kcpad=%d (fwn_cond_stream_rows)", M, cin, kcpad);
    REQUIRE(nsplit >= 1 && nsplit * 8 <= kcpad / 64 * 8 && nsplit <= kcpad / 64 && (nsplit == 1 || (part && part_stride >= (int64_t)nflow * L * M * 512)),
            "fwn_cond_stream: nsplit=%d needs a partial buffer and at most one split per 64-wide chunk", nsplit);
    fwn_launch_cond_rs(ca, ca_odd, Ws, P, nflow * L, L, M, cin, kcpad, part, (long)part_stride, nsplit, (hipStream_t)stream);
    return check_launch("fwn_cond_stream");
}

// the tail that serves flow d at M rows
static TailForm desc_tail(const fwn_flow_desc* d, int M) { return fwn_tail_form(M, d->L, d->Ch, d->npt, d->Wts != nullptr); }

int64_t fwn_tail_stream_bytes(int L) { return L > 0 ? (int64_t)fwn_tail_stream_size(L) : 0; }
int fwn_tail_stream_rows(void) { return fwn_tail_stream_min_rows(); }
int fwn_pack_tail_stream(const void* Wskip, const void* Wfinal, int L, void* out, void* stream) {
    REQUIRE(Wskip && Wfinal && out, "fwn_pack_tail_stream: bad argument");
    REQUIRE(fwn_tail_stream_size(L) != 0, "fwn_pack_tail_stream: no register-streamed tail kernel for L = %d", L);
    REQUIRE(ALIGNED16(Wskip) && ALIGNED16(Wfinal) && ALIGNED16(out), "fwn_pack_tail_stream: buffers must be 16-byte aligned");
    fwn_launch_tail_stream_pack(Wskip, Wfinal, out, (hipStream_t)stream);
    return check_launch("fwn_pack_tail_stream");
}

int fwn_pack_tail_stream_jobs(const fwn_tail_stream_job* jobs, int njobs, int L, void* stream) {
    REQUIRE(jobs && njobs > 0 && njobs < 65536, "fwn_pack_tail_stream_jobs: bad argument");
    REQUIRE(fwn_tail_stream_size(L) != 0, "fwn_pack_tail_stream_jobs: no register-streamed tail kernel for L = %d", L);
    fwn_launch_tail_stream_pack_jobs(jobs, njobs, (hipStream_t)stream);
    return check_launch("fwn_pack_tail_stream_jobs");
}

int fwn_tail(const fwn_flow_desc* d, const void* o, float* xa, float* xb, float* partial, int M,
             int inverse, void* scratch, void* stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    REQUIRE(o && xa && xb && M > 0, "fwn_tail: bad argument");
    REQUIRE(scratch || !desc_tail(d, M).scratch, "fwn_tail: M=%d runs the N-split tail: pass scratch [2][M][256] bf16", M);
    REQUIRE(!scratch || ALIGNED16(scratch), "fwn_tail: scratch must be 16-byte aligned");
    fwn_launch_tail(o, (long)M * 256, d->L, d->Wskip, d->bskip, d->Wfinal, d->bfinal, d->Wzero, d->bzero,
                    d->ezero, d->an, xa, xb, partial, M, d->Ch, d->npt, inverse, scratch,
                    scratch ? (char*)scratch + (size_t)M * 512 : nullptr, nullptr, d->Wts, (hipStream_t)stream);
    return check_launch("fwn_tail");
}

int fwn_tail_can_chain(const fwn_flow_desc* d, int M, int with_front) {
    if (!d || M <= 0) return 0;
    const TailForm f = desc_tail(d, M);
    return with_front ? f.front : f.xb_out;
}
// the public counts are upper bounds over the forms that may serve the shape (which one runs depends on the flow's packed
// operands: with or without the fragment stream): callers zero the buffer, a launch writes its first n slots
static int tail_partials_bound(int M, bool front) {
    const int a = fwn_tail_slots(fwn_tail_form(M, 2, 1, 1, false), M, front), b = fwn_tail_slots(fwn_tail_form(M, 2, 1, 1, true), M, front);
    return a > b ? a : b;
}
int fwn_tail_partials_chained(int M, int Ch, int with_front) { return M > 0 ? tail_partials_bound(M, with_front != 0) : 0; }
// exact: the slots the tail of flow d writes at M rows - mode -1: fwn_tail / fwn_tail_train (in place), 0: fwn_tail_chained
// without a next flow, 1: with one
int fwn_tail_partials_desc(const fwn_flow_desc* d, int M, int mode) { return d && M > 0 ? fwn_tail_slots(desc_tail(d, M), M, mode > 0) : 0; }
int fwn_tail_chained(const fwn_flow_desc* d, const fwn_flow_desc* next, const void* o, float* xa, const float* xb, float* xb_out,
                     void* h0_next, float* partial, int M, int Ti, int inverse, void* scratch, void* stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (next && (rc = check_desc(next))) return rc;
    REQUIRE(o && xa && xb && xb_out && xb_out != xb && M > 0 && Ti > 0 && M % Ti == 0, "fwn_tail_chained: bad argument");
    REQUIRE(fwn_tail_can_chain(d, M, next != nullptr), "fwn_tail_chained: the tail at M=%d, Ch=%d cannot chain%s", M, d->Ch, next ? " a front conv" : "");
    REQUIRE(!next || (h0_next && ALIGNED16(h0_next) && next->Wfront3 && next->kf3 > 0 && next->Ch == d->Ch),
            "fwn_tail_chained: next needs Wfront3 / kf3, the same Ch, and h0_next");
    REQUIRE(scratch || !desc_tail(d, M).scratch, "fwn_tail_chained: M=%d runs the N-split tail: pass scratch [2][M][256] bf16", M);
    fwn_tail_chain tc;
    memset(&tc, 0, sizeof(tc));
    tc.xb_out = xb_out;
    if (next) {
        tc.h0_next = h0_next;
        tc.Wfn = next->Wfront3; tc.bfn = next->bfront; tc.an_next = inverse ? nullptr : next->an; tc.kfn = next->kf3;
    }
    tc.Ti = Ti;
    // (xb is read only; the launcher's xb parameter is not written when xb_out is given)
    fwn_launch_tail(o, (long)M * 256, d->L, d->Wskip, d->bskip, d->Wfinal, d->bfinal, d->Wzero, d->bzero, d->ezero, d->an, xa,
                    const_cast<float*>(xb), inverse ? nullptr : partial, M, d->Ch, d->npt, inverse, scratch,
                    scratch ? (char*)scratch + (size_t)M * 512 : nullptr, &tc, d->Wts, (hipStream_t)stream);
    return check_launch("fwn_tail_chained");
}

int fwn_tail_train(const fwn_flow_desc* d, const void* o, int64_t o_stride, float* xa, float* xb, float* partial, int M,
                   void* save_s, void* save_u, float* save_z, void* stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    REQUIRE(o && xa && xb && M > 0 && o_stride >= 0, "fwn_tail_train: bad argument");
    REQUIRE(save_s && save_u && save_z && ALIGNED16(save_s) && ALIGNED16(save_u) && ALIGNED16(save_z),
            "fwn_tail_train: save_s / save_u / save_z (16-byte aligned) required");
    REQUIRE(((int64_t)(d->L - 1) * o_stride + (int64_t)M * 256) * 2 < ((int64_t)1 << 31), "fwn_tail_train: o spans more than 2 GiB");
    fwn_tail_chain tc;
    memset(&tc, 0, sizeof(tc));
    tc.save_s = save_s; tc.save_u = save_u; tc.save_z = save_z;
    fwn_launch_tail(o, (long)o_stride, d->L, d->Wskip, d->bskip, d->Wfinal, d->bfinal, d->Wzero, d->bzero, d->ezero, d->an, xa, xb,
                    partial, M, d->Ch, d->npt, 0, nullptr, nullptr, &tc, d->Wts, (hipStream_t)stream);
    return check_launch("fwn_tail_train");
}

int fwn_tail_partials(int M) { return M > 0 ? tail_partials_bound(M, false) : 0; }

// Chain context of one flow inside a whole-model call (NULL: a flow on its own, everything in place).
struct FlowChain {
    float* xb_out;               // third plane buffer that receives out_b, or NULL (in place)
    const fwn_flow_desc* next;   // the flow whose front conv this flow's tail also computes (same block), or NULL
    int have_h0;                 // the previous flow's tail has already written this flow's h0 into `h0`
    void* h0_next;               // out: the buffer the next flow's h0 was written to (one of h0 / h1), NULL if none
    int n_partial;               // out: log-det partial slots this flow's tail wrote
};
// A flow of a ragged forward pass (fwn_model_forward_ragged): where its tail keeps Z = (log_s | t) [M][2 Ch] fp32 and where
// the per-clip sums of -log_s go ([B][fwn_ragged_logdet_nslot(B)] fp64).
// mom_part: a ragged init pass (fwn_model_forward_init_ragged) - scratch of the masked moments, fwn_ragged_moments_nslot chunks.
// off / cnt: the rows the sums go over, [off / (2 Ch), + cnt / (2 Ch)) of each clip (DEVICE int32 [B], samples; off NULL: 0) -
// (NULL, the lengths) in a ragged pass, each window's (core_off, core_len) in a windowed forward pass, which has no lengths.
struct FlowRagged {
    float* z;
    double* acc;
    double* mom_part;
    const int32_t* off;
    const int32_t* cnt;
};
// One flow's run.  Zero-initialise, then set by name; what stays zero is absent.
struct FlowRun {
    const fwn_flow_desc* d;
    int64_t B, T;
    float* xa; float* xb;
    const void* ca; const float* P;       // exactly one: fused conditioning plane / the flow's hoisted P
    void* h0; void* h1; void* o;
    float* partial;
    int inverse;
    int ddi;                               // 0 none, 1 local two-pass init, 2 moments -> reduce callback (may be NULL) -> tables
    double* mom; fwn_reduce_fn reduce; void* user;
    void* h8a; void* h8b;                  // e4m3 copies of h: the fp8 gate where the flow and the shape have one
    FlowChain* chain;
    unsigned* sync;                        // != NULL: the flow may run as ONE launch (flow_persist.h); zeroed by the caller
    // ragged batch (whole-model passes only): the clips' lengths in samples, on the device; rg: forward passes
    const int32_t* len;
    const FlowRagged* rg;
    void* stream;
};

static int flow_run_impl(const FlowRun& a) {
    const fwn_flow_desc* d = a.d;
    FlowChain* chain = a.chain;
    const int inverse = a.inverse;
    int rc = check_desc(d);
    if (rc) return rc;
    REQUIRE(a.B > 0 && a.T > 0 && a.T % (2 * (int64_t)d->Ch) == 0, "fwn_flow_run: T=%lld not divisible by 2*Ch=%d",
            (long long)a.T, 2 * d->Ch);
    REQUIRE(a.B * a.T < ((int64_t)1 << 31) && (int64_t)d->L * (a.B * a.T / 2) * 512 < ((int64_t)1 << 31),
            "fwn_flow_run: B*T too large (2 GiB per activation buffer)");
    REQUIRE(a.xa && a.xb && a.h0 && a.h1 && a.o, "fwn_flow_run: null buffer");
    REQUIRE((a.ca != nullptr) != (a.P != nullptr), "fwn_flow_run: exactly one of ca / P");
    REQUIRE(!(a.ddi && inverse), "fwn_flow_run: data-dependent init runs in the forward direction only");
    hipStream_t st = (hipStream_t)a.stream;
    const int Ti = (int)(a.T / (2 * d->Ch));
    const int M = (int)(a.B * Ti);
    const ClipRows rows{a.len, (long)a.B, st};
    if (a.ddi == 1) fwn_launch_ddi(a.xa, a.xb, M, d->Ch, d->an, st);
    if (a.ddi == 2) {
        REQUIRE(a.mom, "fwn_flow_run: no moment buffer");
        // ragged: the clips' own rows only, and their number as the count - the planes hold zeros past a clip's end
        // (ClipRows::zero_planes), which the plain kernel would add to the count
        if (a.len) fwn_launch_ddi_moments_ragged(a.xa, a.xb, (long)a.B, Ti, d->Ch, a.len, 2 * d->Ch, a.mom, a.rg->mom_part, st);
        else fwn_launch_ddi_moments(a.xa, a.xb, M, d->Ch, a.mom, st);
        rc = check_launch("fwn_actnorm_moments");
        if (rc) return rc;
        if (a.reduce && a.reduce(a.user, a.mom, 4 * d->Ch + 1, a.stream) != 0)
            return fail(FWN_ERR_ARG, "fwn_model_forward_init: the reduce callback failed");
        fwn_launch_ddi_from_moments(a.mom, d->Ch, d->an, st);
    }
    // ---- the whole flow as ONE launch (flow_persist.h): small M, hoisted conditioning; `sync` zeroed by the caller ----
    if (a.sync && a.P && !a.ddi && !(a.h8a && a.ca) && !(chain && (chain->have_h0 || chain->xb_out)) &&
        fwn_flow_persist_ok(M, d->Ch, d->L, d->npt, d->Wfront2 != nullptr, ((uintptr_t)a.xa & 15) == 0)) {
        const int inside = fwn_flow_persist_front_inside(d->Ch);
        if (!inside)
            fwn_launch_front(a.xa, d->an, d->Wfront, d->Wfront2, d->bfront, a.h0, a.h1, M, Ti, d->Ch, d->kfpad, inverse ? 0 : 1, nullptr, st);
        fwn_launch_flow_persist_desc(d, a.xa, a.xb, a.h0, a.h1, a.o, a.P, inverse ? nullptr : a.partial, a.sync, M, Ti, inverse, inside, st);
        if (chain) { chain->h0_next = nullptr; chain->n_partial = fwn_tail_slots(fwn_tail_form(M, d->L, d->Ch, d->npt, false), M, false); }
        return check_launch("fwn_flow_run_persist");
    }
    // the stages up to the last gate over the h0 / h1 ping-pong and o [L][M][256]; the front conv's scratch is h1
    FlowStages sg;
    memset(&sg, 0, sizeof(sg));
    for (int l = 0; l < d->L; ++l) {
        sg.h[l] = (l & 1) ? a.h1 : a.h0;
        sg.o[l] = (char*)a.o + (size_t)l * M * 256 * 2;
        // fp8 dilated taps for layer l: e4m3 weights packed, the shape has an fp8 kernel, conditioning fused, and the
        // producer of h (VALU front conv: Ch <= 16; res kernel) can write the e4m3 copy
        if (a.h8a && a.h8b && a.ca && d->Wd8[l] && fwn_gate_fp8_ok(M, dilation_of(l)) && (l > 0 || d->Ch <= 16)) sg.h8[l] = (l & 1) ? a.h8b : a.h8a;
    }
    sg.gate_stream = true;
    sg.front_scratch = a.h1;
    sg.have_h0 = chain && chain->have_h0;
    fwn_run_stages(d, sg, a.xa, a.ca, a.P, M, Ti, inverse, rows);
    void* hc = sg.h[d->L - 1];                          // the last gate's input
    void* hn = hc == a.h0 ? a.h1 : a.h0;
    // both h buffers are free once the last gate has run: the N-split tail (small M) keeps S and U there
    fwn_tail_chain tc;
    memset(&tc, 0, sizeof(tc));
    if (chain) {
        tc.xb_out = chain->xb_out;
        chain->h0_next = nullptr;
        if (chain->next && chain->xb_out) {      // the next flow's front conv rides this tail: its h0 goes to the buffer S does not use
            const fwn_flow_desc* nx = chain->next;
            tc.h0_next = hc;
            tc.Wfn = nx->Wfront3; tc.bfn = nx->bfront; tc.an_next = inverse ? nullptr : nx->an; tc.kfn = nx->kf3; tc.Ti = Ti;
            chain->h0_next = hc;
        }
        chain->n_partial = fwn_tail_slots(desc_tail(d, M), M, tc.h0_next != nullptr);
    }
    // ragged forward: the saving tail (fwn_tail_train's), S and U parked in the two free h buffers, Z kept for the per-clip sums
    if (a.rg) { tc.save_s = hn; tc.save_u = hc; tc.save_z = a.rg->z; }
    fwn_launch_tail(a.o, (long)M * 256, d->L, d->Wskip, d->bskip, d->Wfinal, d->bfinal, d->Wzero, d->bzero,
                    d->ezero, d->an, a.xa, a.xb, inverse ? nullptr : a.partial, M, d->Ch, d->npt, inverse, hn, hc, (chain || a.rg) ? &tc : nullptr,
                    d->Wts, st);
    if (a.rg) fwn_launch_range_logdet(a.rg->z, (long)a.B, Ti, d->Ch, d->ezero, d->an, a.rg->off, a.rg->cnt, (int)a.B, 2 * d->Ch, a.rg->acc, st);
    return check_launch("fwn_flow_run");
}

// the arguments the three single-flow entry points share
static FlowRun flow_run_args(const fwn_flow_desc* d, int64_t B, int64_t T, float* xa, float* xb, void* h0, void* h1, void* o, const float* P,
                             float* partial, int inverse, void* stream) {
    FlowRun a;
    memset(&a, 0, sizeof(a));
    a.d = d; a.B = B; a.T = T; a.xa = xa; a.xb = xb; a.h0 = h0; a.h1 = h1; a.o = o; a.P = P; a.partial = partial; a.inverse = inverse;
    a.stream = stream;
    return a;
}
int fwn_flow_run(const fwn_flow_desc* d, int64_t B, int64_t T, float* xa, float* xb, const void* ca,
                 void* h0, void* h1, void* o, const float* P, float* partial, int inverse, int ddi,
                 void* stream) {
    FlowRun a = flow_run_args(d, B, T, xa, xb, h0, h1, o, P, partial, inverse, stream);
    a.ca = ca; a.ddi = ddi ? 1 : 0;
    return flow_run_impl(a);
}
int fwn_flow_run_fp8(const fwn_flow_desc* d, int64_t B, int64_t T, float* xa, float* xb, const void* ca,
                     void* h0, void* h1, void* o, const float* P, float* partial, int inverse, int ddi,
                     void* h8a, void* h8b, void* stream) {
    REQUIRE(h8a && h8b && ALIGNED16(h8a) && ALIGNED16(h8b), "fwn_flow_run_fp8: h8 scratch buffers (16-byte aligned) required");
    FlowRun a = flow_run_args(d, B, T, xa, xb, h0, h1, o, P, partial, inverse, stream);
    a.ca = ca; a.ddi = ddi ? 1 : 0; a.h8a = h8a; a.h8b = h8b;
    return flow_run_impl(a);
}

int fwn_flow_persist_supported(const fwn_flow_desc* d, int64_t B, int64_t T) {
    if (!d || check_desc(d) != FWN_OK || B <= 0 || T <= 0 || T % (2 * (int64_t)d->Ch) != 0) return 0;
    const int64_t M = B * (T / (2 * d->Ch));
    if (M > ((int64_t)1 << 30)) return 0;
    return fwn_flow_persist_ok((int)M, d->Ch, d->L, d->npt, d->Wfront2 != nullptr, true);
}
int64_t fwn_flow_persist_sync_bytes(int M, int L) { return (M > 0 && L > 0) ? (int64_t)fwn_flow_persist_sync_words(M, L) * 4 : 0; }
int fwn_flow_run_persist(const fwn_flow_desc* d, int64_t B, int64_t T, float* xa, float* xb, void* h0, void* h1, void* o,
                         const float* P, float* partial, int inverse, void* sync, void* stream) {
    REQUIRE(d && sync && P, "fwn_flow_run_persist: null pointer");
    REQUIRE(fwn_flow_persist_supported(d, B, T) && (((uintptr_t)xa) & 15) == 0,
            "fwn_flow_run_persist: this flow / shape has no one-launch form (fwn_flow_persist_supported)");
    FlowRun a = flow_run_args(d, B, T, xa, xb, h0, h1, o, P, partial, inverse, stream);
    a.sync = (unsigned*)sync;
    return flow_run_impl(a);
}
int fwn_flow_persist_status(const void* sync, void* stream) {
    REQUIRE(sync, "fwn_flow_persist_status: null pointer");
    unsigned w[2] = {0, 0};
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess || hipMemcpy(w, sync, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(FWN_ERR_HIP, "fwn_flow_persist_status: copy failed");
    return (int)w[1];
}
int fwn_set_option(const char* name, int value) {
    REQUIRE(name, "fwn_set_option: null name");
    int* slot = !strcmp(name, "rs_persist") ? &g_fwn_opt_rs_persist : !strcmp(name, "persist_spin_us") ? &g_fwn_opt_persist_spin_us : nullptr;
    REQUIRE(slot, "fwn_set_option: unknown option '%s'", name);
    const int old = *slot;
    *slot = value;
    return old;
}

int fwn_prior_logp(const float* planes, int64_t n, const float* partial, int n_partial, float* out2,
                   void* stream) {
    REQUIRE(planes && out2 && n > 0 && n_partial >= 0 && (partial || n_partial == 0), "fwn_prior_logp: bad argument");
    fwn_launch_prior(planes, (long)n, partial, n_partial, 1.0 / (double)n, out2, (hipStream_t)stream);
    return check_launch("fwn_prior_logp");
}

// ---- mel front-end (the data format on the input side of the path) ------------------------------
int fwn_mel_spectrogram(const float* wav, int64_t B, int64_t T, const float* window, const float* fb, int n_fft,
                        int hop, int n_mels, float ref_level_db, float min_level_db, float* mel, void* stream) {
    REQUIRE(wav && window && fb && mel, "fwn_mel_spectrogram: null pointer");
    REQUIRE(n_fft >= 32 && n_fft <= 4096 && (n_fft & (n_fft - 1)) == 0, "fwn_mel_spectrogram: n_fft=%d must be a power of two in [32, 4096]", n_fft);
    REQUIRE(B > 0 && B < 65536 && hop > 0 && n_mels > 0, "fwn_mel_spectrogram: bad shape");
    REQUIRE(T > n_fft / 2, "fwn_mel_spectrogram: T=%lld must exceed n_fft/2 (reflect padding)", (long long)T);
    REQUIRE(min_level_db < 0.0f, "fwn_mel_spectrogram: min_level_db must be negative");
    fwn_launch_mel(wav, (long)B, (long)T, window, fb, n_fft, hop, n_mels, ref_level_db, min_level_db, mel,
                   (hipStream_t)stream);
    return check_launch("fwn_mel_spectrogram");
}

// ---- training-side primitives --------------------------------------------------------------------
// what fwn_gemm accepts: shared with fwn_gemm_tile, so that the query refuses exactly the descriptors the launch refuses
static int gemm_desc_check(const fwn_gemm_desc* g) {
    REQUIRE(g && g->W && g->Y, "fwn_gemm: null pointer");
    REQUIRE(g->nseg >= 1 && g->nseg <= FWN_GEMM_MAXSEG, "fwn_gemm: nseg=%d", g->nseg);
    REQUIRE(g->M > 0 && g->N > 0 && g->ldw > 0 && g->ldy >= g->N && g->Ti >= 0, "fwn_gemm: bad shape");
    REQUIRE(ALIGNED16(g->W) && g->ldw % 8 == 0, "fwn_gemm: W rows must be 16-byte aligned");
    for (int s = 0; s < g->nseg; ++s) {
        const fwn_gemm_seg& sg = g->seg[s];
        REQUIRE(sg.x && sg.k > 0 && sg.k % 8 == 0 && sg.ld >= sg.k && sg.ld % 8 == 0 && ALIGNED16(sg.x) && sg.koff % 8 == 0 &&
                    sg.koff >= 0 && sg.koff + sg.k <= g->ldw && sg.rows > 0,
                "fwn_gemm: segment %d: k, ld, koff must be multiples of 8 within the operands", s);
        REQUIRE((int64_t)sg.rows * sg.ld * 2 < ((int64_t)1 << 31), "fwn_gemm: segment %d exceeds 2 GiB", s);
    }
    REQUIRE((int64_t)g->N * g->ldw * 2 < ((int64_t)1 << 31), "fwn_gemm: W exceeds 2 GiB");
    REQUIRE((int64_t)g->M * g->ldy * (g->out_f32 ? 4 : 2) < ((int64_t)1 << 31) &&
                (!g->R || (int64_t)g->M * g->ldr * 2 < ((int64_t)1 << 31)) &&
                (!g->mask || (int64_t)g->M * g->ldmask * 2 < ((int64_t)1 << 31)),
            "fwn_gemm: output / residual / mask exceed 2 GiB (32-bit buffer offsets)");
    REQUIRE(!g->R || g->ldr >= g->N, "fwn_gemm: ldr < N");
    REQUIRE(!g->mask || g->ldmask >= g->N, "fwn_gemm: ldmask < N");
    REQUIRE(g->nsplit >= 1 && g->nsplit <= 1024, "fwn_gemm: nsplit=%d", g->nsplit);
    REQUIRE(g->nsplit == 1 || (g->out_f32 && !g->bias && !g->R && !g->mask && !g->relu && !g->accumulate),
            "fwn_gemm: split-K writes plain fp32 partials");
    REQUIRE(!g->accumulate || g->out_f32, "fwn_gemm: accumulate needs an fp32 output");
    REQUIRE(!g->gate_aux || (g->gate_out && !g->out_f32 && g->gate_col0 >= 0 && g->gate_col0 % 256 == 0 && g->gate_col0 + 256 <= g->N &&
                             (int64_t)g->M * 512 * 2 < ((int64_t)1 << 31)),
            "fwn_gemm: gate_aux needs gate_out, a bf16 output and 256 columns from gate_col0 (a multiple of 256) inside N");
    REQUIRE(!g->row_len || (g->Ti > 0 && g->M % g->Ti == 0 && g->len_spr > 0 && g->nsplit == 1),
            "fwn_gemm: row_len needs clips (Ti > 0, M a multiple of Ti), len_spr > 0 and no split-K");
    REQUIRE(!g->row_len || !g->accumulate, "fwn_gemm: row_len is refused together with accumulate");
    return FWN_OK;
}
int fwn_gemm(const fwn_gemm_desc* g, void* stream) {
    const int rc = gemm_desc_check(g);
    if (rc != FWN_OK) return rc;
    fwn_gemm_launch(g, (hipStream_t)stream);
    return check_launch("fwn_gemm");
}
int fwn_gemm_tile(const fwn_gemm_desc* g) { return gemm_desc_check(g) == FWN_OK ? fwn_gemm_tile_rule(g) : -1; }
int fwn_transpose_shift(const void* src, int M, int C, int ld_src, int shift0, int dshift, int ntap, int Ti, void* dst,
                        int ld_dst, int ones_row, void* stream) {
    REQUIRE(src && dst && M > 0 && C > 0 && ld_src >= C && ld_dst >= M && Ti >= 0 && ntap >= 1 && ntap <= 64,
            "fwn_transpose_shift: bad argument");
    fwn_transpose_launch(src, M, C, ld_src, shift0, dshift, ntap, Ti, dst, ld_dst, ones_row, (hipStream_t)stream);
    return check_launch("fwn_transpose_shift");
}
int fwn_reduce_splits(const float* partial, int nsplit, int64_t stride, int64_t n, float scale, float* out,
                      void* stream) {
    REQUIRE(partial && out && nsplit >= 1 && n > 0 && stride >= n, "fwn_reduce_splits: bad argument");
    fwn_reduce_splits_launch(partial, nsplit, (long)stride, (long)n, scale, out, (hipStream_t)stream);
    return check_launch("fwn_reduce_splits");
}

int fwn_actnorm_apply(float* x, const float* an, int64_t n, int Ch, void* stream) {
    REQUIRE(x && an && n > 0 && Ch >= 1 && (Ch & (Ch - 1)) == 0, "fwn_actnorm_apply: bad argument");
    fwn_ew_actnorm_fwd(x, an, (long)n, Ch, (hipStream_t)stream);
    return check_launch("fwn_actnorm_apply");
}
int fwn_actnorm_apply2(float* xa, float* xb, const float* an2, int64_t n, int Ch, void* stream) {
    REQUIRE(xa && xb && an2 && n > 0 && Ch >= 1 && (Ch & (Ch - 1)) == 0, "fwn_actnorm_apply2: bad argument");
    fwn_ew_actnorm_fwd2(xa, xb, an2, (long)n, Ch, (hipStream_t)stream);
    return check_launch("fwn_actnorm_apply2");
}
int fwn_coupling_fwd(float* yb, const float* Z, const float* ez, int64_t M, int Ch, float* partial, int nblocks,
                     void* stream) {
    REQUIRE(yb && Z && ez && partial && M > 0 && Ch >= 1 && nblocks >= 1, "fwn_coupling_fwd: bad argument");
    fwn_ew_coupling_fwd(yb, Z, ez, (long)M * Ch, Ch, partial, nblocks, (hipStream_t)stream);
    return check_launch("fwn_coupling_fwd");
}
int fwn_coupling_bwd(float* g, float* out_b, const float* Z, const float* ez, int64_t M, int Ch, float cls, void* dZ,
                     int ldz, float* dzz, void* stream) {
    REQUIRE(g && out_b && Z && ez && dZ && dzz && M > 0 && Ch >= 1 && ldz >= 2 * Ch, "fwn_coupling_bwd: bad argument");
    fwn_ew_coupling_bwd(g, out_b, Z, ez, (long)M * Ch, Ch, cls, dZ, ldz, dzz, (hipStream_t)stream);
    return check_launch("fwn_coupling_bwd");
}
int fwn_coupling_bwd_ragged(float* g, float* out_b, const float* Z, const float* ez, int64_t B, int64_t rows, int Ch, const int32_t* len,
                            int32_t samples_per_row, void* dZ, int ldz, float* dzz, const float* ya, void* ya_bf, int ldya, void* stream) {
    REQUIRE(g && out_b && Z && ez && dZ && dzz && len && B > 0 && rows > 0 && Ch >= 1 && ldz >= 2 * Ch && samples_per_row > 0,
            "fwn_coupling_bwd_ragged: bad argument");
    REQUIRE((ya != nullptr) == (ya_bf != nullptr) && (!ya_bf || ldya >= Ch), "fwn_coupling_bwd_ragged: ya and ya_bf go together, ldya >= Ch");
    REQUIRE(rows <= ((int64_t)1 << 31) / samples_per_row && B * rows * ldz < ((int64_t)1 << 40), "fwn_coupling_bwd_ragged: shape too large");
    fwn_ew_coupling_bwd_ragged(g, out_b, Z, ez, (long)B, (long)rows, Ch, len, samples_per_row, dZ, ldz, dzz, ya, ya_bf, ldya, (hipStream_t)stream);
    return check_launch("fwn_coupling_bwd_ragged");
}
int fwn_gate_bwd(const void* d_o, int ld_do, const void* aux, int64_t M, void* dpre, void* stream) {
    REQUIRE(d_o && aux && dpre && M > 0 && ld_do >= 256, "fwn_gate_bwd: bad argument");
    fwn_ew_gate_bwd(d_o, ld_do, aux, (long)M * 256, dpre, (hipStream_t)stream);
    return check_launch("fwn_gate_bwd");
}
int fwn_colsum_partials(int64_t M, int C_) { return fwn_colsum_blocks((long)M, C_) * C_; }
int fwn_colsum_prod(const float* A, const float* B, int64_t M, int C_, float scale, float* partial, float* out,
                    void* stream) {
    REQUIRE(A && out && partial && M > 0 && C_ > 0, "fwn_colsum_prod: bad argument");
    fwn_ew_colsum_prod(A, B, (long)M, C_, scale, partial, out, (hipStream_t)stream);
    return check_launch("fwn_colsum_prod");
}
int fwn_actnorm_bwd(float* dy, float* y, const float* an, int64_t n, int Ch, void* stream) {
    REQUIRE(dy && y && an && n > 0 && Ch >= 1 && (Ch & (Ch - 1)) == 0, "fwn_actnorm_bwd: bad argument");
    fwn_ew_actnorm_bwd(dy, y, an, (long)n, Ch, (hipStream_t)stream);
    return check_launch("fwn_actnorm_bwd");
}
int64_t fwn_flow_small_grads_partials(int64_t M, int Ch) {
    if (M <= 0 || Ch <= 0) return 0;
    return (int64_t)fwn_small_grads_blocks((long)M, Ch) * 6 * Ch;
}
int fwn_flow_small_grads(float* ga, float* ya, float* gb, float* yb, const float* dzz, const float* an, int64_t M, int Ch,
                         const int64_t* br, const int64_t* zc, double* partial, float* db, float* dlogs, float* dzscale,
                         void* stream) {
    REQUIRE(ga && ya && gb && yb && dzz && an && br && zc && partial && db && dlogs && dzscale, "fwn_flow_small_grads: null pointer");
    REQUIRE(M > 0 && Ch >= 1 && Ch <= 128 && (Ch & (Ch - 1)) == 0, "fwn_flow_small_grads: Ch must be a power of two <= 128");
    fwn_small_grads_launch(ga, ya, gb, yb, dzz, an, (long)M, Ch, (const long long*)br, (const long long*)zc, partial, db, dlogs,
                           dzscale, (hipStream_t)stream);
    return check_launch("fwn_flow_small_grads");
}
int fwn_flow_small_grads_ragged(float* ga, float* ya, float* gb, float* yb, const float* dzz, const float* an, int64_t B, int64_t rows,
                                int Ch, const int32_t* len, int32_t samples_per_row, const int64_t* br, const int64_t* zc, double* partial,
                                float* db, float* dlogs, float* dzscale, void* stream) {
    REQUIRE(ga && ya && gb && yb && dzz && an && len && br && zc && partial && db && dlogs && dzscale, "fwn_flow_small_grads_ragged: null pointer");
    REQUIRE(B > 0 && rows > 0 && samples_per_row > 0 && Ch >= 1 && Ch <= 128 && (Ch & (Ch - 1)) == 0,
            "fwn_flow_small_grads_ragged: Ch must be a power of two <= 128");
    fwn_small_grads_main_ragged(ga, ya, gb, yb, dzz, an, (long)B, (long)rows, Ch, len, samples_per_row, partial, (hipStream_t)stream);
    fwn_small_grads_final(an, (long)(B * rows), Ch, (const long long*)br, (const long long*)zc, partial, db, dlogs, dzscale, (hipStream_t)stream);
    return check_launch("fwn_flow_small_grads_ragged");
}
static bool wn_job_ok(const fwn_wn_job& q) {
    return q.part && q.dV && q.K > 0 && q.N > 0 && q.nsplit >= 1 && q.col0 >= 0 && q.ldp >= q.col0 + q.N && (!q.g || (q.V && q.dg));
}
int64_t fwn_wn_group_scratch(const fwn_wn_job* jobs, int njobs) {
    if (!jobs || njobs < 1 || njobs > FWN_MAX_GROUP) return 0;
    return (int64_t)fwn_wn_group_scratch_doubles(jobs, njobs);
}
int fwn_wn_backward_group(const fwn_wn_job* jobs, int njobs, double* scratch, void* stream) {
    REQUIRE(jobs && njobs >= 1 && njobs <= FWN_MAX_GROUP, "fwn_wn_backward_group: 1..FWN_MAX_GROUP jobs");
    bool any_g = false;
    for (int j = 0; j < njobs; ++j) {
        REQUIRE(wn_job_ok(jobs[j]), "fwn_wn_backward_group: bad job (null pointer, shape, or weight norm without V / dg)");
        any_g = any_g || jobs[j].g;
    }
    REQUIRE(!any_g || scratch, "fwn_wn_backward_group: weight norm needs the scratch buffer");
    fwn_wn_group_launch(jobs, njobs, scratch, (hipStream_t)stream);
    return check_launch("fwn_wn_backward_group");
}

int fwn_upsample_bwd_partials(int B, int H, int s) { return fwn_up_bwd_chunks(B, H) * (6 * s + 1); }
int fwn_upsample_bwd(float* dy, const float* y, const float* x, int B, int H, int W, int s, const float* wk,
                     float* dx, float* dwk_bias, float* partial, void* stream) {
    REQUIRE(dy && y && x && wk && dwk_bias && partial, "fwn_upsample_bwd: null pointer");
    REQUIRE(B > 0 && H > 0 && W > 0 && s > 0 && (s % 2) == 0, "fwn_upsample_bwd: bad shape (s must be even)");
    fwn_up_bwd_launch(dy, y, x, B, H, W, s, wk, dx, dwk_bias, partial, (hipStream_t)stream);
    return check_launch("fwn_upsample_bwd");
}

static const char* tn_job_error(const fwn_tn_job& q, int M) {
    if (!(q.x && q.dy && q.part && q.Kx > 0 && q.N > 0 && q.ntap >= 1 && q.nsplit >= 1)) return "bad argument";
    if (!(q.ldx >= q.Kx && q.ldy >= q.N && q.ldx % 8 == 0 && q.ldy % 8 == 0 && q.Kx % 8 == 0 && q.N % 8 == 0 && ALIGNED16(q.x) &&
          ALIGNED16(q.dy)))
        return "rows must be 16-byte aligned and Kx, N multiples of 8";
    if (!((int64_t)M * q.ldx * 2 < ((int64_t)1 << 31) && (int64_t)M * q.ldy * 2 < ((int64_t)1 << 31) &&
          (int64_t)q.ntap * q.Kx * q.N * 4 < ((int64_t)1 << 31)))
        return "operand exceeds 2 GiB";
    if (!(q.nsplit == 1 || q.split_stride >= ((int64_t)q.ntap * q.Kx + (q.bias_row ? 1 : 0)) * q.N)) return "split_stride too small";
    return nullptr;
}
int fwn_tn_gemm_tile(int M) { return fwn_tn_tile(M); }
int fwn_tn_gemm_group(const fwn_tn_job* jobs, int njobs, int M, int Ti, void* stream) {
    REQUIRE(jobs && njobs >= 1 && njobs <= FWN_MAX_GROUP && M > 0 && Ti >= 0, "fwn_tn_gemm_group: 1..FWN_MAX_GROUP jobs, M > 0");
    for (int j = 0; j < njobs; ++j) {
        const char* e = tn_job_error(jobs[j], M);
        if (e) return fail(FWN_ERR_ARG, "fwn_tn_gemm_group: job %d: %s", j, e);
    }
    fwn_tn_group_launch(jobs, njobs, M, Ti, (hipStream_t)stream);
    return check_launch("fwn_tn_gemm_group");
}
int fwn_tn_gemm(const void* x, int ldx, int Kx, int ntap, int shift0, int dshift, const void* dy, int ldy, int N, int M,
                int Ti, int nsplit, float* part, int64_t split_stride, int bias_row, void* stream) {
    const fwn_tn_job q{x, dy, part, split_stride, ldx, Kx, ntap, shift0, dshift, ldy, N, nsplit, bias_row, 0};
    REQUIRE(M > 0 && Ti >= 0, "fwn_tn_gemm: bad argument");
    const char* e = tn_job_error(q, M);
    if (e) return fail(FWN_ERR_ARG, "fwn_tn_gemm: %s", e);
    fwn_tn_group_launch(&q, 1, M, Ti, (hipStream_t)stream);
    return check_launch("fwn_tn_gemm");
}
int fwn_colsum_bf16(const void* dy, int64_t M, int C_, int ld, float scale, float* partial, float* out, void* stream) {
    REQUIRE(dy && partial && out && M > 0 && C_ > 0 && ld >= C_, "fwn_colsum_bf16: bad argument");
    fwn_colsum_bf16_launch(dy, (long)M, C_, ld, scale, partial, out, (hipStream_t)stream);
    return check_launch("fwn_colsum_bf16");
}

// ---- data-parallel optimiser step -------------------------------------------------------------
int fwn_grad_norm_partials(int64_t n) { return fwn_sqnorm_blocks((long)n); }

int fwn_grad_norm(const float* g, int64_t n, float gscale, double* partial, float* gnorm_out, void* stream) {
    REQUIRE(g && partial && gnorm_out && n > 0, "fwn_grad_norm: bad argument");
    REQUIRE(ALIGNED16(g), "fwn_grad_norm: gradient buffer must be 16-byte aligned");
    fwn_launch_grad_norm(g, (long)n, gscale, partial, gnorm_out, (hipStream_t)stream);
    return check_launch("fwn_grad_norm");
}

int fwn_clip_adam(float* w, const float* g, float* m, float* v, int64_t n, const float* gnorm, float gscale,
                  float clip, float lr, int64_t step, float beta1, float beta2, float eps, void* stream) {
    REQUIRE(w && g && m && v && gnorm && n > 0, "fwn_clip_adam: bad argument");
    REQUIRE(ALIGNED16(w) && ALIGNED16(g) && ALIGNED16(m) && ALIGNED16(v), "fwn_clip_adam: buffers must be 16-byte aligned");
    REQUIRE(step >= 1 && clip > 0.0f && lr > 0.0f, "fwn_clip_adam: step must be >= 1, clip and lr positive");
    const double lr_t = (double)lr * sqrt(1.0 - pow((double)beta2, (double)step)) / (1.0 - pow((double)beta1, (double)step));
    fwn_launch_adam(w, g, m, v, (long)n, gnorm, gscale, clip, (float)lr_t, nullptr, beta1, beta2, eps, (hipStream_t)stream);
    return check_launch("fwn_clip_adam");
}
double fwn_adam_rate(float lr, int64_t step, float beta1, float beta2) {
    return (double)lr * sqrt(1.0 - pow((double)beta2, (double)step)) / (1.0 - pow((double)beta1, (double)step));
}
int fwn_clip_adam_dev(float* w, const float* g, float* m, float* v, int64_t n, const float* gnorm, float gscale,
                      float clip, const float* lr_t, float beta1, float beta2, float eps, void* stream) {
    REQUIRE(w && g && m && v && gnorm && lr_t && n > 0, "fwn_clip_adam_dev: bad argument");
    REQUIRE(ALIGNED16(w) && ALIGNED16(g) && ALIGNED16(m) && ALIGNED16(v), "fwn_clip_adam_dev: buffers must be 16-byte aligned");
    REQUIRE(clip > 0.0f, "fwn_clip_adam_dev: clip must be positive");
    fwn_launch_adam(w, g, m, v, (long)n, gnorm, gscale, clip, 0.0f, lr_t, beta1, beta2, eps, (hipStream_t)stream);
    return check_launch("fwn_clip_adam_dev");
}
int fwn_grad_accumulate(float* dst, const float* a, const float* b, int64_t n, void* stream) {
    REQUIRE(dst && b, "fwn_grad_accumulate: dst and b must not be NULL");
    REQUIRE(n > 0, "fwn_grad_accumulate: n must be positive");
    REQUIRE(!(((uintptr_t)dst | (uintptr_t)a | (uintptr_t)b) & 3), "fwn_grad_accumulate: pointers must be 4-byte aligned");
    // in place (dst == a or dst == b) every element is read and written by one lane; any other overlap with dst would let one
    // lane read what another has already written
    const uintptr_t d0 = (uintptr_t)dst, bytes = (uintptr_t)n * 4;
    for (const float* src : {a, b}) {
        const uintptr_t s0 = (uintptr_t)src;
        REQUIRE(!src || s0 == d0 || s0 + bytes <= d0 || d0 + bytes <= s0, "fwn_grad_accumulate: dst overlaps a source without being it");
    }
    fwn_launch_grad_accumulate(dst, a, b, (long)n, (hipStream_t)stream);
    return check_launch("fwn_grad_accumulate");
}

// ---------------------------------------------------------------------------------------------
// Whole-model sequencing
// ---------------------------------------------------------------------------------------------
static size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

// Inference's hoisting rule (training keeps its own, train_api.hip: it hoists below 4096 rows whatever cin - on purpose, the
// two differ).  cond_mode 1: never, 2: always.
static bool hoist_cond(const fwn_model_desc* m, int64_t M, int cin) {
    if (m->cond_mode == 1) return false;
    if (m->cond_mode == 2) return true;
    // small-M blocks: batch the weight-streaming cond GEMMs of all flows - where the conditioning K is long enough to pay for
    // the extra launch and the P round trip
    constexpr int FWN_HOIST_M = 4096, FWN_HOIST_CIN = 256;
    return M < FWN_HOIST_M && cin >= FWN_HOIST_CIN;
}

// What a whole-model pass runs for one block, decided once per (m, B, T) by carve(): the workspace sizing, the conditioning
// launch, the flow loop and fwn_model_persist_status all read it.
struct BlockPlan {
    int64_t M;               // rows of the block's matrices
    fwn_cond_plan cond;      // hoisted conditioning (cond.hoist) and the launch that computes it
    bool one_launch;         // its flows run as one launch each (flow_persist.h)
    bool chained;            // a flow of it that runs as a launch per stage chains with the next one (flow_chain)
    int slots;               // log-det partial slots reserved per flow: its tail runs plain or chained (overlapping tiles)
};

// whether block b's flows run as one launch each (flow_persist.h); d: its first flow
static bool persist_block(const fwn_model_desc* m, const BlockPlan& b, const fwn_flow_desc* d) {
    // 0: where it measured ahead of the launch-per-stage path (<= 512 rows: blocks 4 - 7 of one clip, block 7 of the 8-clip
    // pass - there with one level's worth of workgroups, flow_persist.h's launcher), 1: nowhere,
    // 2: wherever the form exists.  Same results bit for bit either way.
    if (m->persist_mode == 1) return false;       // (gate_fp8 models too: fp8 taps need fused conditioning and >= 12288 rows - never these blocks)
    constexpr int FWN_PERSIST_AUTO_ROWS = 512;
    if (m->persist_mode != 2 && b.M > FWN_PERSIST_AUTO_ROWS) return false;
    return b.cond.hoist && fwn_flow_persist_ok((int)b.M, d->Ch, d->L, d->npt, d->Wfront2 != nullptr, true);
}

static int check_model(const fwn_model_desc* m, int64_t B, int64_t T) {
    REQUIRE(m && m->flows, "model desc is null");
    REQUIRE(m->n_block >= 1 && m->n_block <= 16 && m->n_flow >= 1 && m->n_layer >= 1 &&
            m->n_layer <= FWN_MAX_LAYERS, "model desc: bad n_block/n_flow/n_layer");
    REQUIRE(m->n_up >= 1 && m->n_up <= FWN_MAX_UPSAMPLE, "model desc: n_up=%d", m->n_up);
    REQUIRE(m->num_mels > 0 && m->num_mels % 2 == 0, "model desc: num_mels must be even");
    REQUIRE(B > 0 && T > 0, "B and T must be positive");
    REQUIRE(T % hop_of(m) == 0, "T=%lld must be a multiple of hop_size=%d (model.py:231)", (long long)T, hop_of(m));
    REQUIRE(T % ((int64_t)1 << m->n_block) == 0, "T=%lld must be a multiple of 2^n_block (model.py:226)",
            (long long)T);
    REQUIRE(B * T < ((int64_t)1 << 31), "B*T too large");
    // every activation matrix is addressed through a raw buffer descriptor with 32-bit offsets and
    // an out-of-range sentinel at 2 GiB: the largest one is o = [n_layer][B*T/2][256] bf16.
    REQUIRE((int64_t)m->n_layer * (B * T / 2) * 512 < ((int64_t)1 << 31) &&
                B * T * (int64_t)(m->num_mels / 2) * 2 < ((int64_t)1 << 31),
            "B*T=%lld samples per call exceeds the 2 GiB-per-buffer limit (split the batch)", (long long)(B * T));
    for (int i = 0; i < m->n_block; ++i)
        for (int j = 0; j < m->n_flow; ++j) {
            const fwn_flow_desc* d = &m->flows[i * m->n_flow + j];
            int rc = check_desc(d);
            if (rc) return rc;
            REQUIRE(d->Ch == (1 << i) && d->L == m->n_layer && d->cin == (m->num_mels / 2) * (2 << i),
                    "model desc: flow (%d,%d) geometry mismatch", i, j);
        }
    for (int i = 0; i < m->n_up; ++i) REQUIRE(m->up_w[i], "model desc: null upsample kernel");
    return FWN_OK;
}

// ---- plane bookkeeping of the chained flows ----
// The flow state lives in two fp32 planes (even / odd samples).  A chained tail writes out_b to a third buffer (its
// neighbours still read the old rows), so the three buffers rotate: `at[k]` = where logical plane k lives now.
struct Planes {
    float* at[2];
    float* spare;
    float* home[2];
};
static void planes_after_flow(Planes& pl, int p, bool rotated) {     // the flow read b = at[p ^ 1] and wrote out_b to spare
    if (!rotated) return;
    float* nb = pl.spare;
    pl.spare = pl.at[p ^ 1];
    pl.at[p ^ 1] = nb;
}
static int planes_go_home(Planes& pl, size_t plane_bytes, hipStream_t st) {   // back to the canonical buffers (no-op when the rotations cancel)
    auto cp = [&](float* dst, float* src) { return hipMemcpyAsync(dst, src, plane_bytes, hipMemcpyDeviceToDevice, st) == hipSuccess; };
    for (int k = 0; k < 2; ++k) {
        if (pl.at[k] == pl.home[k]) continue;
        if (pl.at[k ^ 1] == pl.home[k]) {            // the other plane sits in this one's home: move it to the spare buffer first
            if (!cp(pl.spare, pl.at[k ^ 1])) return -1;
            float* t = pl.spare; pl.spare = pl.at[k ^ 1]; pl.at[k ^ 1] = t;
        }
        if (!cp(pl.home[k], pl.at[k])) return -1;
        if (pl.spare == pl.home[k]) pl.spare = pl.at[k];
        pl.at[k] = pl.home[k];
    }
    return 0;
}

struct Carve {
    size_t cplanes, up0, up1, planes, plane3, h0, h1, o, P, Ppart, partial, mom, h8a, h8b, sync, mel, zsave, acc, mompart, total;
    size_t sync_stride, sync_bytes;       // one block of counters per flow (flow_persist.h), zeroed once per pass
    BlockPlan blk[16];
};

// The layout of a pass of kind k (pass_traits: what a pass with per-clip lengths adds, behind everything else - the plain
// passes all share one layout).
static Carve carve(const fwn_model_desc* m, int64_t B, int64_t T, PassKind k) {
    const PassTraits pt = pass_traits(k);
    Carve c;
    size_t off = 0;
    const size_t half = m->num_mels / 2;
    c.cplanes = off; off = align_up(off + 2 * (size_t)B * T * half * 2);
    const size_t up_elems = (m->n_up > 1) ? (size_t)B * (T / m->up_scale[m->n_up - 1]) * m->num_mels : 0;
    c.up0 = off; off = align_up(off + up_elems * 4);
    c.up1 = off; off = align_up(off + (m->n_up > 2 ? up_elems * 4 : 0));
    c.planes = off; off = align_up(off + (size_t)B * T * 4);
    c.plane3 = off; off = align_up(off + (size_t)B * T * 2);      // third plane buffer: chained flows write out_b beside their inputs
    const size_t Mmax = (size_t)B * T / 2;
    c.h0 = off; off = align_up(off + Mmax * 256 * 2);
    c.h1 = off; off = align_up(off + Mmax * 256 * 2);
    c.o = off; off = align_up(off + (size_t)m->n_layer * Mmax * 256 * 2);
    size_t pbytes = 0, ppart = 0;
    int npart = 0;
    c.sync_stride = 0;
    for (int i = 0; i < m->n_block; ++i) {
        BlockPlan& b = c.blk[i];
        const fwn_flow_desc* f0 = &m->flows[i * m->n_flow];
        b.M = B * T / ((int64_t)2 << i);
        b.cond = fwn_plan_cond(hoist_cond(m, b.M, f0->cin), (int)b.M, m->n_flow, m->n_layer, f0->cin, f0->kcpad, m->cond_stream[i]);
        b.one_launch = !pt.ragged && persist_block(m, b, f0);
        b.chained = !pt.ragged && m->chain_mode != 1;
        b.slots = fwn_tail_partials_chained((int)b.M, f0->Ch, 1);       // chained with a front conv: the most tiles
        if (b.cond.hoist) {
            const size_t need = (size_t)m->n_flow * m->n_layer * b.M * 512 * 4;
            if (need > pbytes) pbytes = need;
            const size_t sp = (size_t)(b.cond.nsplit - 1) * need;
            if (sp > ppart) ppart = sp;
        }
        npart += m->n_flow * b.slots;
        if (b.one_launch) {
            const size_t w = (size_t)fwn_flow_persist_sync_words((int)b.M, m->n_layer) * 4;
            if (w > c.sync_stride) c.sync_stride = w;
        }
    }
    c.P = off; off = align_up(off + pbytes);
    c.Ppart = off; off = align_up(off + ppart);        // split-K partials of the hoisted conditioning (few rows)
    c.partial = off; off = align_up(off + (size_t)npart * 4);
    // per-flow moment buffers of the data-parallel ActNorm init: 4 Ch + 1 doubles each, Ch <= 2^(n_block-1)
    c.mom = off; off = align_up(off + (size_t)m->n_block * m->n_flow * (4 * ((size_t)1 << (m->n_block - 1)) + 1) * 8);
    c.h8a = off; off = align_up(off + (m->gate_fp8 ? Mmax * 256 : 0));      // e4m3 copies of h (fp8 gate path)
    c.h8b = off; off = align_up(off + (m->gate_fp8 ? Mmax * 256 : 0));
    c.sync_bytes = c.sync_stride * (size_t)m->n_block * m->n_flow;
    c.sync = off; off = align_up(off + c.sync_bytes);
    c.mel = off; off = align_up(off + (pt.ragged ? (size_t)B * (T / hop_of(m)) * m->num_mels * 4 : 0));
    c.zsave = off; off = align_up(off + (pt.logdet ? (size_t)B * T * 4 : 0));          // [M][2 Ch] fp32 = B T floats at every block
    c.acc = off; off = align_up(off + (pt.logdet ? (size_t)m->n_block * m->n_flow * B * fwn_ragged_logdet_nslot((long)B) * 8 : 0));
    size_t mp = 0;
    for (int i = 0; pt.mompart && i < m->n_block; ++i) {
        const size_t need = (size_t)fwn_ragged_moments_nslot((long)B, (long)(T >> (i + 1)), 1 << i) * (4 << i) * 8;
        if (need > mp) mp = need;
    }
    c.mompart = off; off = align_up(off + mp);
    c.total = off;
    return c;
}

size_t fwn_workspace_bytes(const fwn_model_desc* m, int64_t B, int64_t T) {
    if (check_model(m, B, T) != FWN_OK) return 0;
    return carve(m, B, T, PASS_FORWARD).total;
}
size_t fwn_ragged_workspace_bytes(const fwn_model_desc* m, int64_t B, int64_t T) {
    if (check_model(m, B, T) != FWN_OK) return 0;
    return carve(m, B, T, PASS_REVERSE_RAGGED).total;
}
size_t fwn_ragged_forward_workspace_bytes(const fwn_model_desc* m, int64_t B, int64_t T) {
    if (check_model(m, B, T) != FWN_OK || B >= 32768) return 0;
    return carve(m, B, T, PASS_FORWARD_RAGGED).total;
}
size_t fwn_ragged_init_workspace_bytes(const fwn_model_desc* m, int64_t B, int64_t T) {
    if (check_model(m, B, T) != FWN_OK || B >= 32768 || m->gate_fp8) return 0;
    return carve(m, B, T, PASS_INIT_RAGGED).total;
}

static int check_block_contiguity(const fwn_model_desc* m, int blk) {
    const fwn_flow_desc* f0 = &m->flows[blk * m->n_flow];
    const size_t stride = (size_t)512 * f0->kcpad * 2;
    for (int j = 0; j < m->n_flow; ++j)
        for (int l = 0; l < m->n_layer; ++l)
            REQUIRE((const char*)m->flows[blk * m->n_flow + j].Wc[l] ==
                        (const char*)f0->Wc[0] + (size_t)(j * m->n_layer + l) * stride,
                    "block %d: Wc must be contiguous in (flow, layer) order for hoisted conditioning", blk);
    return FWN_OK;
}

// What flow `d` chains with inside a whole-model call: out_b to the spare plane wherever the tail at this shape can write
// it elsewhere, and the front conv of `next` (the flow that runs after d in this block and direction) in d's tail where
// that kernel exists (Ch <= 8) - not during the data-dependent init (next's ActNorm table does not exist yet) and not on
// the fp8 path (its first gate reads an e4m3 copy of h0 that only the stand-alone front conv writes).
static FlowChain flow_chain(const fwn_model_desc* m, const fwn_flow_desc* d, const fwn_flow_desc* next, int M, bool init, float* spare,
                            int have_h0, bool chained) {
    FlowChain ch;
    memset(&ch, 0, sizeof(ch));
    // (a block whose flows run as ONE launch each - flow_persist.h - does not chain: that form holds the whole flow already;
    // BlockPlan.chained)
    const bool on = chained;
    const TailForm f = desc_tail(d, M);
    ch.xb_out = (on && f.xb_out) ? spare : nullptr;
    ch.next = (ch.xb_out && next && !init && !m->gate_fp8 && next->Wfront3 && next->kf3 > 0 && f.front) ? next : nullptr;
    ch.have_h0 = have_h0;
    return ch;
}

static int record_block_event(const fwn_model_desc* m, int k, hipStream_t st) {
    if (!m->block_events || !m->block_events[k]) return 0;
    return hipEventRecord((hipEvent_t)m->block_events[k], st) != hipSuccess;
}

// Whether any one-launch flow of the LAST pass run in `workspace` (fwn_model_forward / fwn_model_reverse with the same m, B, T)
// gave up a bounded dependency wait (its outputs are NaN then: never silently wrong, but the pass itself returned FWN_OK):
// 0 = none, > 0 = the give-up code of the first such flow (1 + the stage that waited).  Synchronises the stream.  ADVICE r5: the
// per-flow sync blocks live inside the workspace, out of reach of fwn_flow_persist_status.
int fwn_model_persist_status(const fwn_model_desc* m, int64_t B, int64_t T, const void* workspace, void* stream) {
    int rc = check_model(m, B, T);
    if (rc) return rc;
    REQUIRE(workspace, "fwn_model_persist_status: null workspace");
    const Carve c = carve(m, B, T, PASS_FORWARD);
    if (!c.sync_bytes) return 0;
    const int nf = m->n_block * m->n_flow;
    unsigned w[1024];
    REQUIRE(nf <= 1024, "fwn_model_persist_status: more than 1024 flows");
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess ||
        hipMemcpy2D(w, sizeof(unsigned), (const char*)workspace + c.sync + sizeof(unsigned), c.sync_stride, sizeof(unsigned), (size_t)nf,
                    hipMemcpyDeviceToHost) != hipSuccess)
        return fail(FWN_ERR_HIP, "fwn_model_persist_status: copy failed");
    for (int k = 0; k < nf; ++k)
        if (w[k]) return (int)w[k];
    return 0;
}

// One pass over the blocks and flows in either direction.  Forward: blocks and flows in order, the parity flipped after each
// flow (change_order, model.py:190); it collects the log-det partials and runs the data-dependent init (init 1: local, 2:
// moments -> reduce callback), and ends in the prior.  Reverse: both orders backwards, the parity flipped before each flow
// (model.py:199); it ends in the merge of the planes into x_out.  A block's plan (carve) decides its conditioning launch and
// whether its flows run as one launch each; the init pass runs no flow as one launch, but zeroes the sync region all the same.
// kind (fwn_sequence.h) names the entry point; pass_traits gives its direction, its init and what per-clip lengths add.
// A ragged pass (len): the same stages under the plan of carve(.., kind), with the rows past each clip's end zeroed wherever
// a later stage reads across it: mel and inner up-sampling stages (fwn_run_upsample), planes, h (fwn_run_stages), and x_out.
// Forward with len: every flow's x_a plane gets -shift in those rows before its front conv and its tail keeps Z (flow_run_impl),
// the per-clip log-det sums of all flows and the per-clip prior end in out2 [2][B] (the tails' own partials are ignored).
// PASS_INIT_RAGGED: that pass with init 2 - every flow's moments over the clips' own rows.
// PASS_FORWARD_WINDOWS (wc): the ragged forward's form - a launch per stage, every tail keeps Z - on full-length rows, so no
// fill or mask is launched (len NULL); each flow's -log_s sums go over the window's core rows, and the pass ends with the planes
// at home in the workspace: the prior, the per-clip sums and the latent are the caller's (fwn_model_forward_windows).
struct WindowCores {
    const int32_t* off;      // DEVICE int32 [B]: each window's core, in samples from the window's start
    const int32_t* len;
};
static int model_pass(PassKind kind, const fwn_model_desc* m, int64_t B, int64_t T, const float* in, const float* mel, const int32_t* len,
                      void* workspace, size_t workspace_bytes, fwn_reduce_fn reduce, void* user, float* out2, float* z_planes, float* x_out,
                      void* stream, const WindowCores* wc = nullptr) {
    const PassTraits pt = pass_traits(kind);
    const char* what = pt.what;
    const bool reverse = pt.reverse;
    const int init = pt.init;
    int rc = check_model(m, B, T);
    if (rc) return rc;
    REQUIRE(in && mel && workspace && (reverse ? (void*)x_out : wc ? (void*)wc->off : (void*)out2), "%s: null pointer", what);
    REQUIRE((((uintptr_t)workspace) & 255) == 0, "workspace must be 256-byte aligned");
    REQUIRE(!reverse || ((m->n_block * m->n_flow) & 1) == 0,
            "reverse with odd n_block*n_flow ends in swapped channel order (model.py:199,254); unsupported");
    REQUIRE(!pt.ragged || !m->gate_fp8,
            "%s: per-clip lengths go with a model without fp8 gates (its e4m3 copies of h are not masked) and without the data-dependent init", what);
    const Carve c = carve(m, B, T, kind);
    if (workspace_bytes < c.total)
        return fail(FWN_ERR_WORKSPACE, "workspace %zu < required %zu bytes", workspace_bytes, c.total);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const size_t half = m->num_mels / 2;
    const size_t cplane_bytes = (size_t)B * T * half * 2;
    const size_t plane_elems = (size_t)B * T / 2;
    const size_t mom_stride = 4 * ((size_t)1 << (m->n_block - 1)) + 1;
    float* planes = (float*)(ws + c.planes);
    const int nf = m->n_flow, L = m->n_layer;

    const ClipRows rows{len, (long)B, st};
    {
        UpsampleBufs u;
        memset(&u, 0, sizeof(u));
        u.mel_copy = (float*)(ws + c.mel);
        for (int i = 0; i + 1 < m->n_up; ++i) u.inner[i] = (float*)(ws + ((i & 1) ? c.up1 : c.up0));
        u.cplanes = ws + c.cplanes;
        if (fwn_run_upsample(m, (long)B, (long)T, mel, u, rows)) return fail(FWN_ERR_HIP, "%s: mel copy failed", what);
    }
    fwn_launch_split(in, B, T, planes, st);   // (reverse: the n_block pre-squeezes of model.py:374-392 are index math)
    // ragged batch: both planes hold clip b's samples at [b][0, len / 2) at every block (a row of block i is 2^i of them, and
    // len is a multiple of 2^n_block); the rest is zeroed here and behind every flow (ActNorm^-1 and the coupling leave -b
    // and t there, and the next front conv reads one row across the clip's end)
    rows.zero_planes(planes, (long)T);
    if (c.sync_bytes && hipMemsetAsync(ws + c.sync, 0, c.sync_bytes, st) != hipSuccess)
        return fail(FWN_ERR_HIP, "%s: hipMemsetAsync failed", what);
    int p = 0;
    float* partial = reverse ? nullptr : (float*)(ws + c.partial);
    int poff = 0;
    Planes pl{{planes, planes + plane_elems}, (float*)(ws + c.plane3), {planes, planes + plane_elems}};
    for (int k = 0; k < m->n_block; ++k) {
        if (record_block_event(m, k, st)) return fail(FWN_ERR_HIP, "%s: hipEventRecord failed", what);
        const int i = reverse ? m->n_block - 1 - k : k;
        const BlockPlan& b = c.blk[i];
        const int M = (int)b.M;
        const fwn_flow_desc* f0 = &m->flows[i * nf];
        if (b.cond.hoist) {
            rc = check_block_contiguity(m, i);
            if (rc) return rc;
            // the plane flows 0 and 1 read: the parity flips once per flow, after it (forward) or before it (reverse)
            const int par0 = reverse ? p ^ (nf & 1) : p, par1 = reverse ? p ^ ((nf - 1) & 1) : p ^ 1;
            fwn_run_cond(b.cond, ws + c.cplanes + (size_t)par0 * cplane_bytes, ws + c.cplanes + (size_t)par1 * cplane_bytes, f0->Wc[0],
                         (float*)(ws + c.P), (float*)(ws + c.Ppart), M, nf, L, f0->cin, f0->kcpad, st);
        }
        void* hA = ws + c.h0;
        void* hB = ws + c.h1;
        int have_h0 = 0;
        for (int n = 0; n < nf; ++n) {
            const int j = reverse ? nf - 1 - n : n;
            if (reverse) p ^= 1;
            const fwn_flow_desc* d = &m->flows[i * nf + j];
            const fwn_flow_desc* next = reverse ? (j > 0 ? d - 1 : nullptr) : (j + 1 < nf ? d + 1 : nullptr);
            const void* ca = b.cond.hoist ? nullptr : (const void*)(ws + c.cplanes + (size_t)p * cplane_bytes);
            const float* P = b.cond.hoist ? (const float*)(ws + c.P) + (size_t)j * L * M * 512 : nullptr;
            double* mom = (double*)(ws + c.mom) + (size_t)(i * nf + j) * mom_stride;
            unsigned* sync = (!init && b.one_launch) ? (unsigned*)(ws + c.sync + (size_t)(i * nf + j) * c.sync_stride) : nullptr;
            FlowChain ch = flow_chain(m, d, next, M, init != 0, pl.spare, have_h0, b.chained && !sync);
            const FlowRagged rg{(float*)(ws + c.zsave), (double*)(ws + c.acc) + (size_t)(i * nf + j) * B * fwn_ragged_logdet_nslot((long)B),
                                pt.mompart ? (double*)(ws + c.mompart) : nullptr, wc ? wc->off : nullptr, wc ? wc->len : len};
            FlowRun fr;
            memset(&fr, 0, sizeof(fr));
            fr.d = d; fr.B = B; fr.T = T; fr.xa = pl.at[p]; fr.xb = pl.at[p ^ 1]; fr.ca = ca; fr.P = P;
            fr.h0 = hA; fr.h1 = hB; fr.o = ws + c.o;
            fr.partial = reverse ? nullptr : partial + poff;
            fr.inverse = reverse; fr.ddi = init; fr.mom = mom; fr.reduce = reduce; fr.user = user;
            if (m->gate_fp8) { fr.h8a = ws + c.h8a; fr.h8b = ws + c.h8b; }
            fr.chain = &ch; fr.sync = sync; fr.len = len;
            if (pt.logdet) fr.rg = &rg;
            fr.stream = stream;
            rc = flow_run_impl(fr);
            if (rc) return rc;
            rows.zero_planes(planes, (long)T);
            if (!reverse) poff += ch.n_partial;
            planes_after_flow(pl, p, ch.xb_out != nullptr);
            have_h0 = ch.h0_next != nullptr;
            if (have_h0 && ch.h0_next != hA) { void* t = hA; hA = hB; hB = t; }
            if (!reverse) p ^= 1;
        }
    }
    if (record_block_event(m, m->n_block, st)) return fail(FWN_ERR_HIP, "%s: hipEventRecord failed", what);
    if (planes_go_home(pl, plane_elems * 4, st)) return fail(FWN_ERR_HIP, "%s: plane copy failed", what);
    if (reverse) {
        fwn_launch_merge(planes, B, T, x_out, st);
        rows.zero(x_out, (long)T, 4, 1);
    } else {
        if (wc) return check_launch(what);
        if (len) fwn_launch_ragged_finish(planes, (long)B, (long)T, (const double*)(ws + c.acc), m->n_block * nf, nf, len, out2, st);
        else fwn_launch_prior(planes, (long)(B * T), partial, poff, 1.0 / (double)(B * T), out2, st);
        if (z_planes) {
            hipError_t e = hipMemcpyAsync(z_planes, planes, (size_t)B * T * 4, hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) return fail(FWN_ERR_HIP, "hipMemcpyAsync: %s", hipGetErrorString(e));
        }
    }
    return check_launch(what);
}

int fwn_model_forward(const fwn_model_desc* m, int64_t B, int64_t T, const float* x, const float* mel,
                      void* workspace, size_t workspace_bytes, float* out2, float* z_planes, int init,
                      void* stream) {
    return model_pass(init ? PASS_FORWARD_DDI : PASS_FORWARD, m, B, T, x, mel, nullptr, workspace, workspace_bytes, nullptr, nullptr, out2,
                      z_planes, nullptr, stream);
}
int fwn_model_forward_init(const fwn_model_desc* m, int64_t B, int64_t T, const float* x, const float* mel,
                           void* workspace, size_t workspace_bytes, float* out2, float* z_planes,
                           fwn_reduce_fn reduce, void* user, void* stream) {
    return model_pass(PASS_FORWARD_INIT, m, B, T, x, mel, nullptr, workspace, workspace_bytes, reduce, user, out2, z_planes, nullptr, stream);
}

int fwn_model_reverse(const fwn_model_desc* m, int64_t B, int64_t T, const float* z, const float* mel,
                      void* workspace, size_t workspace_bytes, float* x_out, void* stream) {
    return model_pass(PASS_REVERSE, m, B, T, z, mel, nullptr, workspace, workspace_bytes, nullptr, nullptr, nullptr, nullptr, x_out, stream);
}
int fwn_model_reverse_ragged(const fwn_model_desc* m, int64_t B, int64_t T, const float* z, const float* mel, const int32_t* len_dev,
                             void* workspace, size_t workspace_bytes, float* x_out, void* stream) {
    REQUIRE(len_dev, "fwn_model_reverse_ragged: null lengths");
    REQUIRE(B < 32768, "fwn_model_reverse_ragged: B=%lld clips (at most 32767 per call)", (long long)B);
    return model_pass(PASS_REVERSE_RAGGED, m, B, T, z, mel, len_dev, workspace, workspace_bytes, nullptr, nullptr, nullptr, nullptr, x_out,
                      stream);
}
int fwn_model_forward_ragged(const fwn_model_desc* m, int64_t B, int64_t T, const float* x, const float* mel, const int32_t* len_dev,
                             void* workspace, size_t workspace_bytes, float* out2B, float* z_planes, void* stream) {
    REQUIRE(len_dev, "fwn_model_forward_ragged: null lengths");
    REQUIRE(B < 32768, "fwn_model_forward_ragged: B=%lld clips (at most 32767 per call)", (long long)B);
    return model_pass(PASS_FORWARD_RAGGED, m, B, T, x, mel, len_dev, workspace, workspace_bytes, nullptr, nullptr, out2B, z_planes, nullptr,
                      stream);
}

int fwn_model_forward_init_ragged(const fwn_model_desc* m, int64_t B, int64_t T, const float* x, const float* mel, const int32_t* len_dev,
                                  void* workspace, size_t workspace_bytes, float* out2B, float* z_planes, fwn_reduce_fn reduce, void* user,
                                  void* stream) {
    REQUIRE(len_dev, "fwn_model_forward_init_ragged: null lengths");
    REQUIRE(B < 32768, "fwn_model_forward_init_ragged: B=%lld clips (at most 32767 per call)", (long long)B);
    return model_pass(PASS_INIT_RAGGED, m, B, T, x, mel, len_dev, workspace, workspace_bytes, reduce, user, out2B, z_planes, nullptr, stream);
}

// ---- device-side synthesis: z drawn on the device -> the inverse pass -> 16-bit PCM (include/fwn.h) ----
int fwn_latent_normal(float* z, int64_t B, int64_t T, uint64_t seed, const uint32_t* clip_id_dev, float temp, const int32_t* len_dev,
                      void* stream) {
    REQUIRE(z && B > 0 && B < 65536 && T > 0, "fwn_latent_normal: bad argument");
    REQUIRE((((uintptr_t)z) & 3) == 0, "fwn_latent_normal: z must be 4-byte aligned");
    REQUIRE(T <= ((int64_t)1 << 34), "fwn_latent_normal: T=%lld exceeds the 2^32 quads one clip's counter word numbers", (long long)T);
    fwn_launch_latent_normal_at(z, (long)B, (long)T, (unsigned long long)seed, clip_id_dev, nullptr, temp, len_dev, (hipStream_t)stream);
    return check_launch("fwn_latent_normal");
}
int fwn_pcm16(const float* x, int16_t* pcm, int64_t B, int64_t T, const int32_t* len_dev, void* stream) {
    REQUIRE(x && pcm && B > 0 && B < 65536 && T > 0, "fwn_pcm16: bad argument");
    REQUIRE((((uintptr_t)x) & 3) == 0 && (((uintptr_t)pcm) & 1) == 0, "fwn_pcm16: x must be 4-byte and pcm 2-byte aligned");
    fwn_launch_pcm16(x, (short*)pcm, (long)B, (long)T, len_dev, (hipStream_t)stream);
    return check_launch("fwn_pcm16");
}
// the inverse pass's own workspace first (so model_pass carves it as ever), then z and the waveform, B T floats each
static size_t synth_extra(int64_t B, int64_t T) { return align_up((size_t)B * T * 4); }
size_t fwn_synthesize_workspace_bytes(const fwn_model_desc* m, int64_t B, int64_t T, int ragged) {
    if (check_model(m, B, T) != FWN_OK || B >= 32768 || (ragged && m->gate_fp8)) return 0;
    return carve(m, B, T, ragged ? PASS_REVERSE_RAGGED : PASS_REVERSE).total + 2 * synth_extra(B, T);
}
int fwn_model_synthesize(const fwn_model_desc* m, int64_t B, int64_t T, const float* mel, uint64_t seed, const uint32_t* clip_id_dev,
                         float temp, const int32_t* len_dev, void* workspace, size_t workspace_bytes, int16_t* pcm_out, float* wav_out,
                         float* z_out, void* stream) {
    // everything the inverse pass would refuse is refused here, before the latent fill is enqueued
    int rc = check_model(m, B, T);
    if (rc) return rc;
    REQUIRE(mel && workspace && pcm_out, "fwn_model_synthesize: null pointer");
    REQUIRE((((uintptr_t)workspace) & 255) == 0, "fwn_model_synthesize: workspace must be 256-byte aligned");
    REQUIRE(ALIGNED16(pcm_out) && ALIGNED16(wav_out) && ALIGNED16(z_out), "fwn_model_synthesize: pcm_out, wav_out and z_out must be 16-byte aligned");
    REQUIRE(B < 32768, "fwn_model_synthesize: B=%lld clips (at most 32767 per call)", (long long)B);
    REQUIRE(((m->n_block * m->n_flow) & 1) == 0,
            "fwn_model_synthesize: reverse with odd n_block*n_flow ends in swapped channel order (model.py:199,254); unsupported");
    REQUIRE(!len_dev || !m->gate_fp8,
            "fwn_model_synthesize: per-clip lengths go with a model without fp8 gates (its e4m3 copies of h are not masked)");
    const PassKind kind = len_dev ? PASS_REVERSE_RAGGED : PASS_REVERSE;
    const size_t base = carve(m, B, T, kind).total, extra = synth_extra(B, T);
    if (workspace_bytes < base + 2 * extra)
        return fail(FWN_ERR_WORKSPACE, "fwn_model_synthesize: workspace %zu < required %zu bytes", workspace_bytes, base + 2 * extra);
    float* z = z_out ? z_out : (float*)((char*)workspace + base);
    float* wav = wav_out ? wav_out : (float*)((char*)workspace + base + extra);
    fwn_launch_latent_normal_at(z, (long)B, (long)T, (unsigned long long)seed, clip_id_dev, nullptr, temp, len_dev, (hipStream_t)stream);
    rc = check_launch("fwn_model_synthesize (latent)");
    if (rc) return rc;
    rc = model_pass(kind, m, B, T, z, mel, len_dev, workspace, base, nullptr, nullptr, nullptr, nullptr, wav, stream);
    if (rc) return rc;
    fwn_launch_pcm16(wav, (short*)pcm_out, (long)B, (long)T, len_dev, (hipStream_t)stream);
    return check_launch("fwn_model_synthesize");
}

// ---- windowed synthesis: one group of n windows of L samples - latent slices, mel rows, the inverse pass, the cores (include/fwn.h) ----
int fwn_latent_normal_at(float* z, int64_t n, int64_t L, uint64_t seed, const uint32_t* clip_id_dev, const int64_t* start_dev, float temp,
                         const int32_t* len_dev, void* stream) {
    REQUIRE(z && start_dev && n > 0 && n < 65536 && L > 0, "fwn_latent_normal_at: bad argument");
    REQUIRE(ALIGNED4(z) && ALIGNED4(clip_id_dev) && ALIGNED4(len_dev), "fwn_latent_normal_at: z, clip_id_dev and len_dev must be 4-byte aligned");
    REQUIRE(ALIGNED8(start_dev), "fwn_latent_normal_at: start_dev must be 8-byte aligned");
    REQUIRE(L <= ((int64_t)1 << 34), "fwn_latent_normal_at: L=%lld exceeds the 2^32 quads one clip's counter word numbers", (long long)L);
    fwn_launch_latent_normal_at(z, (long)n, (long)L, (unsigned long long)seed, clip_id_dev, (const long long*)start_dev, temp, len_dev,
                                (hipStream_t)stream);
    return check_launch("fwn_latent_normal_at");
}
int fwn_window_gather(const float* src, const int64_t* src_row_dev, float* dst, int64_t n, int64_t rows, int64_t row_floats, void* stream) {
    REQUIRE(src && src_row_dev && dst, "fwn_window_gather: null pointer");
    REQUIRE(n > 0 && n < 65536 && rows > 0 && row_floats > 0, "fwn_window_gather: n, rows and row_floats must be positive, n < 65536");
    REQUIRE(rows < ((int64_t)1 << 31) && row_floats < ((int64_t)1 << 31) && rows * row_floats < ((int64_t)1 << 31),
            "fwn_window_gather: a window of %lld rows of %lld floats exceeds 2^31 elements", (long long)rows, (long long)row_floats);
    REQUIRE(ALIGNED4(src) && ALIGNED4(dst), "fwn_window_gather: src and dst must be 4-byte aligned");
    REQUIRE(ALIGNED8(src_row_dev), "fwn_window_gather: src_row_dev must be 8-byte aligned");
    fwn_launch_window_gather(src, (const long long*)src_row_dev, (long)row_floats, dst, (long)n, (long)(rows * row_floats), (hipStream_t)stream);
    return check_launch("fwn_window_gather");
}
int fwn_window_scatter_pcm16(const float* x, int64_t n, int64_t L, const int32_t* core_off_dev, const int32_t* core_len_dev,
                             const int64_t* out_off_dev, int16_t* pcm, float* wav, void* stream) {
    REQUIRE(x && core_off_dev && core_len_dev && out_off_dev && (pcm || wav), "fwn_window_scatter_pcm16: null pointer");
    REQUIRE(n > 0 && n < 65536 && L > 0 && L < ((int64_t)1 << 31), "fwn_window_scatter_pcm16: n in [1, 65535] and L in [1, 2^31)");
    REQUIRE(ALIGNED4(x) && ALIGNED4(wav) && (((uintptr_t)pcm) & 1) == 0 && ALIGNED4(core_off_dev) && ALIGNED4(core_len_dev),
            "fwn_window_scatter_pcm16: x, wav and the int32 tables must be 4-byte, pcm 2-byte aligned");
    REQUIRE(ALIGNED8(out_off_dev), "fwn_window_scatter_pcm16: out_off_dev must be 8-byte aligned");
    fwn_launch_window_scatter(x, (long)n, (long)L, core_off_dev, core_len_dev, (const long long*)out_off_dev, (short*)pcm, wav,
                              (hipStream_t)stream);
    return check_launch("fwn_window_scatter_pcm16");
}
// the inverse pass's own workspace first (so model_pass carves it as ever), then z, the waveform and the windows' mel rows:
// all of (n, L) alone
static size_t windows_mel_bytes(const fwn_model_desc* m, int64_t n, int64_t L) {
    return align_up((size_t)n * (size_t)(L / hop_of(m)) * m->num_mels * 4);
}
// what both group entries (`who`) refuse alike: the model and the shape (check_model), more than 32 767 windows, a workspace
// off its 256 bytes, an 8-byte buffer (the int64 tables, fp64) or a 4-byte one (the 32-bit tables, fp32) off its alignment.
// A NULL is aligned: whether it may be one is the entry's own check.
static int check_windows_call(const char* who, const fwn_model_desc* m, int64_t n, int64_t L, const void* workspace,
                              std::initializer_list<const void*> b8, std::initializer_list<const void*> b4) {
    int rc = check_model(m, n, L);
    if (rc) return rc;
    REQUIRE(n < 32768, "%s: n=%lld windows (at most 32767 per call)", who, (long long)n);
    REQUIRE((((uintptr_t)workspace) & 255) == 0, "%s: workspace must be 256-byte aligned", who);
    for (const void* p : b8) REQUIRE(ALIGNED8(p), "%s: the int64 tables and fp64 buffers must be 8-byte aligned", who);
    for (const void* p : b4) REQUIRE(ALIGNED4(p), "%s: the 32-bit tables and fp32 buffers must be 4-byte aligned", who);
    return FWN_OK;
}
size_t fwn_synthesize_windows_workspace_bytes(const fwn_model_desc* m, int64_t n, int64_t L) {
    if (check_model(m, n, L) != FWN_OK || n >= 32768 || ((m->n_block * m->n_flow) & 1)) return 0;
    return carve(m, n, L, PASS_REVERSE).total + 2 * synth_extra(n, L) + windows_mel_bytes(m, n, L);
}
int fwn_model_synthesize_windows(const fwn_model_desc* m, int64_t n, int64_t L, const float* mel_flat, const int64_t* mel_row_dev,
                                 const uint32_t* clip_id_dev, const int64_t* start_dev, const int32_t* core_off_dev,
                                 const int32_t* core_len_dev, const int64_t* out_off_dev, uint64_t seed, float temp, void* workspace,
                                 size_t workspace_bytes, int16_t* pcm_flat, float* wav_flat, void* stream) {
    // everything the inverse pass would refuse is refused here, before the latent fill is enqueued
    int rc = check_windows_call("fwn_model_synthesize_windows", m, n, L, workspace, {mel_row_dev, start_dev, out_off_dev},
                                {clip_id_dev, core_off_dev, core_len_dev, mel_flat, wav_flat});
    if (rc) return rc;
    REQUIRE(mel_flat && workspace && pcm_flat, "fwn_model_synthesize_windows: null pointer");
    REQUIRE(mel_row_dev && clip_id_dev && start_dev && core_off_dev && core_len_dev && out_off_dev, "fwn_model_synthesize_windows: null table");
    REQUIRE((((uintptr_t)pcm_flat) & 1) == 0, "fwn_model_synthesize_windows: pcm_flat must be 2-byte aligned");
    REQUIRE(((m->n_block * m->n_flow) & 1) == 0,
            "fwn_model_synthesize_windows: reverse with odd n_block*n_flow ends in swapped channel order (model.py:199,254); unsupported");
    const size_t base = carve(m, n, L, PASS_REVERSE).total, extra = synth_extra(n, L), need = base + 2 * extra + windows_mel_bytes(m, n, L);
    if (workspace_bytes < need)
        return fail(FWN_ERR_WORKSPACE, "fwn_model_synthesize_windows: workspace %zu < required %zu bytes", workspace_bytes, need);
    float* z = (float*)((char*)workspace + base);
    float* wav = (float*)((char*)workspace + base + extra);
    float* mel = (float*)((char*)workspace + base + 2 * extra);
    hipStream_t st = (hipStream_t)stream;
    fwn_launch_latent_normal_at(z, (long)n, (long)L, (unsigned long long)seed, clip_id_dev, (const long long*)start_dev, temp, nullptr, st);
    fwn_launch_window_gather(mel_flat, (const long long*)mel_row_dev, (long)m->num_mels, mel, (long)n, (long)(L / hop_of(m)) * m->num_mels, st);
    rc = check_launch("fwn_model_synthesize_windows (latent, mel rows)");
    if (rc) return rc;
    rc = model_pass(PASS_REVERSE, m, n, L, z, mel, nullptr, workspace, base, nullptr, nullptr, nullptr, nullptr, wav, stream);
    if (rc) return rc;
    fwn_launch_window_scatter(wav, (long)n, (long)L, core_off_dev, core_len_dev, (const long long*)out_off_dev, (short*)pcm_flat, wav_flat, st);
    return check_launch("fwn_model_synthesize_windows");
}

// ---- windowed forward: one group of n windows of L samples - audio and mel rows, the pass, the cores' sums and latent (include/fwn.h) ----
int fwn_window_logdet_rows(const float* Z, int64_t n, int64_t rows, int Ch, const float* ez, const float* an, const int32_t* core_off_dev,
                           const int32_t* core_len_dev, int32_t samples_per_row, double* acc, void* stream) {
    REQUIRE(Z && ez && core_off_dev && core_len_dev && acc && n > 0 && n < 65536 && rows > 0 && samples_per_row > 0,
            "fwn_window_logdet_rows: bad argument");
    REQUIRE(Ch >= 1 && (Ch & (Ch - 1)) == 0, "fwn_window_logdet_rows: Ch=%d must be a power of two", Ch);
    REQUIRE(ALIGNED4(Z) && ALIGNED8(acc) && ALIGNED4(core_off_dev) && ALIGNED4(core_len_dev), "fwn_window_logdet_rows: misaligned buffer");
    REQUIRE(rows <= ((int64_t)1 << 31) / samples_per_row, "fwn_window_logdet_rows: rows * samples_per_row exceeds 2^31");
    fwn_launch_range_logdet(Z, (long)n, (long)rows, Ch, ez, an, core_off_dev, core_len_dev, (int)n, samples_per_row, acc, (hipStream_t)stream);
    return check_launch("fwn_window_logdet_rows");
}
int fwn_window_sums(const float* planes, int64_t n, int64_t L, const int32_t* core_off_dev, const int32_t* core_len_dev, const double* acc,
                    int nflows, int n_flow, const int32_t* slot_dev, double* part, void* stream) {
    REQUIRE(planes && core_off_dev && core_len_dev && acc && slot_dev && part, "fwn_window_sums: null pointer");
    REQUIRE(n > 0 && n < 65536 && L > 0 && L < ((int64_t)1 << 31) && L % 2 == 0 && nflows >= 0 && n_flow >= 1,
            "fwn_window_sums: n in [1, 65535], L even in [2, 2^31), nflows >= 0, n_flow >= 1");
    REQUIRE(ALIGNED4(planes) && ALIGNED4(core_off_dev) && ALIGNED4(core_len_dev) && ALIGNED4(slot_dev) && ALIGNED8(acc) && ALIGNED8(part),
            "fwn_window_sums: misaligned buffer");
    fwn_launch_window_sums(planes, (long)n, (long)L, core_off_dev, core_len_dev, acc, nflows, n_flow, slot_dev, part, (hipStream_t)stream);
    return check_launch("fwn_window_sums");
}
int fwn_window_scatter_latent(const float* planes, int64_t n, int64_t L, int swapped, const int32_t* core_off_dev,
                              const int32_t* core_len_dev, const int64_t* out_off_dev, float* z_flat, void* stream) {
    REQUIRE(planes && core_off_dev && core_len_dev && out_off_dev && z_flat, "fwn_window_scatter_latent: null pointer");
    REQUIRE(n > 0 && n < 65536 && L > 0 && L < ((int64_t)1 << 31) && L % 2 == 0, "fwn_window_scatter_latent: n in [1, 65535], L even in [2, 2^31)");
    REQUIRE(ALIGNED4(planes) && ALIGNED4(z_flat) && ALIGNED4(core_off_dev) && ALIGNED4(core_len_dev),
            "fwn_window_scatter_latent: planes, z_flat and the int32 tables must be 4-byte aligned");
    REQUIRE(ALIGNED8(out_off_dev), "fwn_window_scatter_latent: out_off_dev must be 8-byte aligned");
    fwn_launch_window_latent(planes, (long)n, (long)L, swapped ? 1 : 0, core_off_dev, core_len_dev, (const long long*)out_off_dev, z_flat,
                             (hipStream_t)stream);
    return check_launch("fwn_window_scatter_latent");
}
int fwn_forward_windows_finish(const double* part, const int32_t* clip_slot0_dev, const int32_t* clip_nwin_dev, int64_t n_clips, float* out2B,
                               void* stream) {
    REQUIRE(part && clip_slot0_dev && clip_nwin_dev && out2B && n_clips > 0 && n_clips < ((int64_t)1 << 31), "fwn_forward_windows_finish: bad argument");
    REQUIRE(ALIGNED8(part) && ALIGNED4(clip_slot0_dev) && ALIGNED4(clip_nwin_dev) && ALIGNED4(out2B), "fwn_forward_windows_finish: misaligned buffer");
    fwn_launch_windows_finish(part, clip_slot0_dev, clip_nwin_dev, (long)n_clips, out2B, (hipStream_t)stream);
    return check_launch("fwn_forward_windows_finish");
}
// the pass's own workspace first (model_pass carves it as ever; its mel region receives the windows' mel rows - a pass without
// lengths reads the mel it is given and never copies it), then the windows' audio
size_t fwn_forward_windows_workspace_bytes(const fwn_model_desc* m, int64_t n, int64_t L) {
    if (check_model(m, n, L) != FWN_OK || n >= 32768 || m->gate_fp8) return 0;
    return carve(m, n, L, PASS_FORWARD_WINDOWS).total + synth_extra(n, L);
}
int fwn_model_forward_windows(const fwn_model_desc* m, int64_t n, int64_t L, const float* x_flat, const int64_t* x_row_dev,
                              const float* mel_flat, const int64_t* mel_row_dev, const int32_t* core_off_dev, const int32_t* core_len_dev,
                              const int32_t* slot_dev, double* acc, const int64_t* z_out_off_dev, float* z_flat, void* workspace,
                              size_t workspace_bytes, void* stream) {
    // everything the pass would refuse is refused here, before the gathers are enqueued
    int rc = check_windows_call("fwn_model_forward_windows", m, n, L, workspace, {x_row_dev, mel_row_dev, z_out_off_dev, acc},
                                {core_off_dev, core_len_dev, slot_dev, x_flat, mel_flat, z_flat});
    if (rc) return rc;
    REQUIRE(x_flat && mel_flat && workspace && acc, "fwn_model_forward_windows: null pointer");
    REQUIRE(x_row_dev && mel_row_dev && core_off_dev && core_len_dev && slot_dev && (z_out_off_dev || !z_flat),
            "fwn_model_forward_windows: null table");
    REQUIRE(!m->gate_fp8, "fwn_model_forward_windows: windows go with a model without fp8 gates (the pass is the ragged forward's form)");
    const Carve c = carve(m, n, L, PASS_FORWARD_WINDOWS);
    const size_t need = c.total + synth_extra(n, L);
    if (workspace_bytes < need)
        return fail(FWN_ERR_WORKSPACE, "fwn_model_forward_windows: workspace %zu < required %zu bytes", workspace_bytes, need);
    char* ws = (char*)workspace;
    float* xg = (float*)(ws + c.total);
    float* mel = (float*)(ws + c.mel);
    hipStream_t st = (hipStream_t)stream;
    const int hop = hop_of(m);
    fwn_launch_window_gather(x_flat, (const long long*)x_row_dev, (long)hop, xg, (long)n, (long)L, st);
    fwn_launch_window_gather(mel_flat, (const long long*)mel_row_dev, (long)m->num_mels, mel, (long)n, (long)(L / hop) * m->num_mels, st);
    rc = check_launch("fwn_model_forward_windows (audio, mel rows)");
    if (rc) return rc;
    const WindowCores wc{core_off_dev, core_len_dev};
    rc = model_pass(PASS_FORWARD_WINDOWS, m, n, L, xg, mel, nullptr, workspace, c.total, nullptr, nullptr, nullptr, nullptr, nullptr, stream, &wc);
    if (rc) return rc;
    const float* planes = (const float*)(ws + c.planes);
    fwn_launch_window_sums(planes, (long)n, (long)L, core_off_dev, core_len_dev, (const double*)(ws + c.acc), m->n_block * m->n_flow,
                           m->n_flow, slot_dev, acc, st);
    if (z_flat)
        fwn_launch_window_latent(planes, (long)n, (long)L, (m->n_block * m->n_flow) & 1, core_off_dev, core_len_dev,
                                 (const long long*)z_out_off_dev, z_flat, st);
    return check_launch("fwn_model_forward_windows");
}

// ---- device-resident corpus: one training batch drawn and gathered on the device (include/fwn.h) ----
int fwn_corpus_draw(const float* audio, const float* mel, const int64_t* frame_off, int64_t n_utt, int hop, int num_mels,
                    int unit_frames, int64_t B, int64_t F, uint64_t seed, uint32_t stream_id, uint64_t* counter_dev, float* x, float* c,
                    int32_t* len, int32_t* picks, void* stream) {
    REQUIRE(audio && mel && frame_off && counter_dev && x && c && len, "fwn_corpus_draw: null pointer");
    REQUIRE(B >= 1 && F >= 1 && n_utt >= 1 && hop >= 1 && num_mels >= 1 && unit_frames >= 1,
            "fwn_corpus_draw: B, F, n_utt, hop, num_mels and unit_frames must be positive (B %lld, F %lld, n_utt %lld, hop %d, num_mels %d, "
            "unit_frames %d)", (long long)B, (long long)F, (long long)n_utt, hop, num_mels, unit_frames);
    REQUIRE(B < 65536, "fwn_corpus_draw: B=%lld slots (at most 65535 per call)", (long long)B);
    REQUIRE(n_utt < ((int64_t)1 << 31), "fwn_corpus_draw: n_utt=%lld utterances (fewer than 2^31)", (long long)n_utt);
    REQUIRE(F * hop < ((int64_t)1 << 31) && F * num_mels < ((int64_t)1 << 31),
            "fwn_corpus_draw: a row of F=%lld frames exceeds 2^31 elements", (long long)F);
    REQUIRE(((((uintptr_t)audio) | ((uintptr_t)mel) | ((uintptr_t)x) | ((uintptr_t)c) | ((uintptr_t)len) | ((uintptr_t)picks)) & 3) == 0,
            "fwn_corpus_draw: audio, mel, x, c, len and picks must be 4-byte aligned");
    REQUIRE(((((uintptr_t)frame_off) | ((uintptr_t)counter_dev)) & 7) == 0, "fwn_corpus_draw: frame_off and counter_dev must be 8-byte aligned");
    fwn_launch_corpus_draw(audio, mel, (const long long*)frame_off, (long)n_utt, hop, num_mels, unit_frames, (long)B, (long)F,
                           (unsigned long long)seed, (unsigned)stream_id, (unsigned long long*)counter_dev, x, c, len, picks,
                           (hipStream_t)stream);
    return check_launch("fwn_corpus_draw");
}

}  // extern "C"
