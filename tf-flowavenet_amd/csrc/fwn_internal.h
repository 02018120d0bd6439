// Internal launcher prototypes shared by the kernel translation units and api.hip.
#pragma once
#include <hip/hip_runtime.h>

// h8out (may be NULL): also write the e4m3 copy of the output the fp8 gate reads (front: Ch <= 16 only)
void fwn_launch_front(const float* xa, const float* an_a, const void* W, const void* W2, const float* bias,
                      void* hout, void* scratch, int M, int Ti, int Ch, int kpad, int apply_an, void* h8out, hipStream_t st);
// Wgs: the same weights in fragment order (fwn_launch_gate_stream_pack) or nullptr; used instead of Wd / Wc where
// fwn_gate_stream_ok says so
int fwn_launch_gate_clock(const void* h, const void* ca, const void* Wgs, const float* bias, void* o, int M, int Ti, int dil, int cin,
                          unsigned long long* clk, hipStream_t st);
// Wds: Wd alone in the conditioning kernel's fragment order (fwn_launch_cond_stream_pack, kcpad = 768) or nullptr; used with a
// hoisted P where fwn_gate_hs_ok says so
void fwn_launch_gate(const void* h, const void* ca, const float* P, const void* Wd, const void* Wc, const void* Wgs, const void* Wds,
                     const float* bias, void* o, int M, int Ti, int dil, int cin, int kcpad, void* aux,
                     hipStream_t st);
// The tile launch_ring (flow_kernels.hip) picks for an M x N product: the largest that still yields about one workgroup per CU.
enum fwn_ring_tile { FWN_RING_256x256, FWN_RING_256x128, FWN_RING_128x128, FWN_RING_64x128, FWN_RING_SPLITK };
inline fwn_ring_tile fwn_ring_tile_for(int M, int N, bool allow256) {
    const int FILL = 192;    // workgroups needed before a fatter tile pays (256 CUs)
    if (allow256 && N % 256 == 0 && ((M + 255) / 256) * (N / 256) >= FILL) return FWN_RING_256x256;
    if (((M + 255) / 256) * (N / 128) >= FILL) return FWN_RING_256x128;
    if (((M + 127) / 128) * (N / 128) >= FILL) return FWN_RING_128x128;
    if (((M + 63) / 64) * (N / 128) >= FILL) return FWN_RING_64x128;
    return FWN_RING_SPLITK;  // 64 x 64 tiles, the K range dealt over wave groups (flow_persist_kernel reproduces their partial sums)
}
// cond_rs.hip: the hoisted gate from the fragment stream of Wd (gate_hs_kernel, cond_rs.h).  fwn_gate_hs_ok: the shape is one the
// ring path would give its un-split 64 x 128 tile; rows / cols: the workgroup tile (64 | 96 | 128 rows x 512 | 256 columns),
// 0 / 0 = the shipped one.  Returns the number of workgroups launched, 0 if there is no such tile.
bool fwn_gate_hs_ok(int M, int Ti, int dil);
int fwn_launch_gate_hs(const void* h, const void* Wds, const float* bias, const float* P, void* o, int M, int Ti, int dil,
                       int rows, int cols, hipStream_t st);
// measurement control: the same gate on a given ring tile (rows 64 | 128 | 256, 128 columns); 0 if there is no such tile
int fwn_launch_gate_ring_tile(const void* h, const float* P, const void* Wd, const float* bias, void* o, int M, int Ti, int dil,
                              int rows, hipStream_t st);
long fwn_gate_stream_size(int cin);        // bytes, 0: no kernel for this cin
int fwn_gate_stream_min_rows();
int fwn_gate_stream_ok(int M, int Ti, int dil, int cin, bool fused_cond, bool aux);
void fwn_launch_gate_stream_pack(const void* Wd, const void* Wc, int cin, int kcpad, void* out, hipStream_t st);
// gate_rs.hip: the register-streamed launch itself (the caller has checked fwn_gate_stream_ok)
void fwn_launch_gate_rs(const void* h, const void* ca, const void* Wgs, const float* bias, void* o, int M, int Ti, int dil, int cin,
                        hipStream_t st);
// the gate with its dilated taps in fp8 (h8 e4m3 [M][256], Wd8 e4m3 [512][768] stored as W 2^wexp); fwn_gate_fp8_ok says
// whether this shape has such a kernel (the tap-sharing tiles: M >= 12288 rows, dilation <= 3, conditioning fused)
int fwn_gate_fp8_ok(int M, int dil);
void fwn_launch_gate_fp8(const void* h8, const void* ca, const void* Wd8, int wexp, const void* Wc, const float* bias, void* o,
                         int M, int Ti, int dil, int cin, int kcpad, hipStream_t st);
void fwn_launch_res(const void* o, const void* hin, const void* W, const float* bias, void* hout, int M, void* h8out,
                    hipStream_t st);
void fwn_launch_cond(const void* ca, const void* Wc_base, float* P_base, long w_stride, long p_stride,
                     int flow0, int flow_step, int nflow, int L, int M, int cin, int kcpad, float* part_base, long part_stride,
                     int nsplit, hipStream_t st);
// whether both parity groups of a block go into ONE launch (cheaper by the stream model of flow_kernels.hip, or split K)
bool fwn_cond_merge(int M, int nz_group, int nsplit);
void fwn_launch_cond2(const void* ca, const void* ca_odd, const void* Wc_base, float* P_base, long w_stride, long p_stride,
                      int flow0, int flow_step, int nflow, int L, int M, int cin, int kcpad, float* part_base, long part_stride,
                      int nsplit, hipStream_t st);
// split-K of the hoisted conditioning for few rows: the split count for nz matrices per launch, and the in-order sum of
// the partial outputs (part: [nsplit - 1][..] laid out like P) into P[0..n)
int fwn_cond_nsplit(int M, int nz, int kcpad);
void fwn_launch_cond_reduce(float* P, const float* part, long part_stride, int nsplit, long n, hipStream_t st);
// register-streamed form (cond_rs.h / cond_rs.hip): whole blocks of nz = nflow * L matrices from their fragment streams
long fwn_cond_stream_size(int kcpad);
int fwn_cond_stream_min_rows();
bool fwn_cond_rs_ok(int M, int cin, int kcpad, bool have_stream);               // the kernel serves the shape
bool fwn_cond_rs_wanted(int M, int cin, int kcpad, int nz, bool have_stream);   // ... and the model-level calls use it there
int fwn_cond_rs_nsplit(int M, int nz, int kcpad);
void fwn_launch_cond_stream_pack(const void* Wc_base, long w_stride, int kcpad, int nz, void* out, hipStream_t st);
void fwn_launch_cond_rs(const void* ca, const void* ca_odd, const void* Ws, float* P, int nz, int L, int M, int cin, int kcpad,
                        float* part, long part_stride, int nsplit, hipStream_t st);
// The hoisted conditioning of a block of nflow flows (flow_kernels.hip): which launch computes its P matrices and with how many
// K splits.  The caller decides whether to hoist (inference and training keep different rules); stream: the block's fragment
// stream (fwn_launch_cond_stream_pack) or NULL.  fwn_run_cond launches it: ca0 is the plane even flows read, ca1 the odd flows',
// P [nflow * L][M][512] fp32, Ppart (nsplit - 1) more of the same.
struct fwn_cond_plan {
    bool hoist;             // false: every gate fuses its conditioning (nothing to launch)
    const void* stream;     // != NULL: the register-streamed kernel (cond_rs.h) reads this stream
    bool merged;            // else: both parity groups in one ring launch (fwn_launch_cond2), else one launch per group
    int nsplit;             // K splits
};
fwn_cond_plan fwn_plan_cond(bool hoist, int M, int nflow, int L, int cin, int kcpad, const void* stream);
void fwn_run_cond(const fwn_cond_plan& cp, const void* ca0, const void* ca1, const void* Wc0, float* P, float* Ppart, int M, int nflow,
                  int L, int cin, int kcpad, hipStream_t st);
// Chaining the flows of a block (whole-model calls): out_b to a third plane buffer, and the NEXT flow's front conv computed
// by this tail (csrc/tail_chain.h).  NULL / all-zero = the plain in-place tail.
struct fwn_tail_chain {
    float* xb_out;          // out_b destination; NULL: in place (xb)
    void* h0_next;          // != NULL: also the next flow's h0 [M][256] bf16 (needs xb_out: the tiles then overlap by one row)
    const void* Wfn;        // next flow's chained front weights [256][kfn] (fwn_flow_desc.Wfront3)
    const float* bfn;       // its bias [256]
    const float* an_next;   // forward: the next flow's ActNorm table; inverse: NULL
    int kfn, Ti;
    // what the training backward keeps of the tail (each optional): S = ReLU(skip sum), U = ReLU(final conv) as bf16
    // [M][256] in natural channel order, Z = U Wz + bz as fp32 [M][2 Ch] (log_s channels, then t channels, plane order)
    void* save_s;
    void* save_u;
    float* save_z;
};
void fwn_launch_tail(const void* o, long o_stride, int L, const void* Ws, const float* bs, const void* Wf,
                     const float* bfin, const void* Wz, const float* bz, const float* ez, const float* an,
                     float* xa, float* xb, float* partial, int M, int Ch, int npt, int inverse, void* scratch_s,
                     void* scratch_u, const fwn_tail_chain* chain, const void* Wts, hipStream_t st);
// The one choice of tail kernel for a shape (flow_kernels.hip): fwn_launch_tail runs it, and every log-det slot count, scratch
// check and chaining query of the host derives from it.  have_stream: the flow's fragment stream (Wts) is packed.
enum TailKind {
    TAIL_RS,             // register-streamed (tail_rs.h), rs_mt 32-row tiles per workgroup
    TAIL_FUSED256,       // register-chained tail_kernel (tail_chain.h), 256-row workgroups
    TAIL_FUSED128,       // ... 128-row workgroups
    TAIL_SPLIT_CHAIN,    // N-split: skip-sum ring GEMM, then the chained kernel on 64-row tiles
    TAIL_SPLIT3,         // N-split, three ring GEMM launches
};
struct TailForm {
    TailKind kind;
    int rows;            // rows per workgroup (the log-det slot per workgroup)
    int rs_mt;           // TAIL_RS: 32-row tiles per workgroup, else 0
    bool scratch;        // needs the [2][M][256] bf16 S / U scratch (or training's save_s / save_u)
    bool xb_out;         // can write out_b elsewhere (fwn_tail_chain.xb_out)
    bool front;          // ... and can compute the next flow's front conv (fwn_tail_chain.h0_next)
};
TailForm fwn_tail_form(int M, int L, int Ch, int npt, bool have_stream);
int fwn_tail_slots(const TailForm& f, int M, bool front);   // log-det partial slots one launch writes (front: h0_next set)
// register-streamed tail (tail_rs.h / tail_rs.hip).  Wts: Wskip | Wfinal in fragment order (fwn_launch_tail_stream_pack) or nullptr
struct TailArgs;
long fwn_tail_stream_size(int L);          // bytes, 0: no kernel for this layer count
int fwn_tail_stream_min_rows();
void fwn_launch_tail_stream_pack(const void* Ws, const void* Wf, void* out, hipStream_t st);
void fwn_launch_tail_stream_pack_jobs(const void* jobs, int njobs, hipStream_t st);     // jobs: device array of {Wskip, Wfinal, out}
void fwn_launch_tail_rs(const TailArgs& a, const void* Wts, int mt, hipStream_t st);

// one flow of the small-M chain as one launch (flow_persist.h)
struct fwn_flow_desc;
int fwn_flow_persist_sync_words(int M, int L);
int fwn_flow_persist_ok(int M, int Ch, int L, int npt, bool has_w2, bool xa_aligned);
int fwn_flow_persist_front_inside(int Ch);
void fwn_launch_flow_persist_desc(const fwn_flow_desc* d, float* xa, float* xb, void* hA, void* hB, void* o, const float* P,
                                  float* partial, unsigned* sync, int M, int Ti, int inverse, int has_front, hipStream_t st);
// process-wide developer options (fwn_set_option): -1 = auto
extern int g_fwn_opt_rs_persist;
extern int g_fwn_opt_persist_spin_us;     // flow_persist.h: bound of the one-launch flow's spins in microseconds (0 = 2 s)
int fwn_device_cus();            // compute units of the current device (cached per device)

void fwn_launch_wn_scale(const float* v, const float* g, int k_src, int n_src, float* scale, hipStream_t st);
void fwn_launch_pack(const float* v, const float* scale, const int* src_k, const int* src_n, int n_src,
                     int k_dst, int n_dst, long ld_dst, void* out, hipStream_t st);
void fwn_launch_wn_absmax(const float* v, const float* scale, int k_src, int n_src, float mul, float* amax, hipStream_t st);
void fwn_launch_pack_e4m3(const float* v, const float* scale, const int* src_k, const int* src_n, int n_src, int k_dst,
                          int n_dst, long ld_dst, float mul, const float* amax, void* out, int* exp_out, hipStream_t st);
void fwn_launch_cast_e4m3(const void* src, void* dst, long n, hipStream_t st);
void fwn_launch_gather_tables(const float* flat, const long long* idx, int nterm, long total, const double* post,
                              const unsigned char* expflag, float* out, hipStream_t st);
void fwn_launch_sum_f32(const float* in, long n, float* out, hipStream_t st);
void fwn_launch_upsample_wn(const float* v, const float* g, int s, float* out, hipStream_t st);
void fwn_launch_upsample(const float* in, int B, int H, int W, const float* wk, float bias, const float* bias_dev, int s,
                         float* out_f32, void* out_planes, hipStream_t st);
void fwn_launch_split(const float* x, long B, long T, float* planes, hipStream_t st);
void fwn_launch_merge(const float* planes, long B, long T, float* x, hipStream_t st);
// zero rows [len[c % nlen] / samples_per_row, rows) of every clip c of a [nclip][rows][row_bytes] buffer (ragged batches: the
// rows past a clip's own length); len is read on the device and clamped to the buffer.  base and row_bytes: multiples of 4.
void fwn_launch_mask_rows(void* base, long nclip, long rows, long row_bytes, const int* len, int nlen, int samples_per_row,
                          hipStream_t st);
// synthesis (aux_kernels.hip): fp32 [B][T] -> int16 PCM; len (may be NULL) is read on the device and clamped to [0, T]: 0 from
// there on.
void fwn_launch_pcm16(const float* x, short* pcm, long B, long T, const int* len, hipStream_t st);
// synthesis, whole clips and windows (aux_kernels.hip; fwn.h has the contracts): row r of z [n][L] = temp * N(0,1), samples
// start[r] .. start[r] + L (start NULL: from 0) of the Philox4x32-10 stream keyed by (seed, clip_id[r]) (NULL: clip r is r),
// +0 from len[r] on (may be NULL; clamped to [0, L]); row r of dst [n][count] = count floats of src from src_row[r] *
// row_floats; the core [core_off[r], core_off[r] + core_len[r]) of row r of x [n][L] -> pcm + out_off[r] (int16) and / or
// wav + out_off[r] (fp32).  Every table is read on the device.
void fwn_launch_latent_normal_at(float* z, long n, long L, unsigned long long seed, const unsigned* clip_id, const long long* start,
                                 float temp, const int* len, hipStream_t st);
void fwn_launch_window_gather(const float* src, const long long* src_row, long row_floats, float* dst, long n, long count,
                              hipStream_t st);
void fwn_launch_window_scatter(const float* x, long n, long L, const int* core_off, const int* core_len, const long long* out_off,
                               short* pcm, float* wav, hipStream_t st);
// training data (aux_kernels.hip): slot b of x [B][F hop] / c [B][F][num_mels] / len [B] / picks [B][2] drawn from the flat corpus
// by Philox keyed on (seed, stream_id, *counter, b), then *counter + 1 from one lane of a second launch (fwn.h fwn_corpus_draw)
void fwn_launch_corpus_draw(const float* audio, const float* mel, const long long* frame_off, long n_utt, int hop, int num_mels,
                            int unit_frames, long B, long F, unsigned long long seed, unsigned stream_id, unsigned long long* counter,
                            float* x, float* c, int* len, int* picks, hipStream_t st);
// ragged forward (aux_kernels.hip).  -shift[tau] into rows [len / samples_per_row, rows) of every clip of a [nclip][rows][Ch]
// fp32 plane: the front conv's on-the-fly ActNorm then gives exact zeros there.  Clamped like fwn_launch_mask_rows.
void fwn_launch_fill_neg_shift(float* plane, long nclip, long rows, int Ch, const float* shift, const int* len, int nlen,
                               int samples_per_row, hipStream_t st);
// One flow's log-det terms per clip from the tail's saved Z [nclip][rows][2 Ch]: acc[clip][0 .. nslot - 1) = fp64 chunk sums of
// -log_s over rows [off[clip] / samples_per_row, + cnt[clip % ncnt] / samples_per_row) of the clip - off NULL: from row 0,
// a ragged clip's own rows with cnt its length; a window's core with (core_off, core_len) -, acc[clip][nslot - 1] = sum_tau
// of the ActNorm's 3 logs (both planes; an may be NULL); nslot = fwn_ragged_logdet_nslot(nclip).  fwn_launch_ragged_finish
// turns acc [nflows][nclip][nslot] and the planes into out2B [2][nclip] = per-clip (log_p, logdet).
int fwn_ragged_logdet_nslot(long nclip);
void fwn_launch_range_logdet(const float* Z, long nclip, long rows, int Ch, const float* ez, const float* an, const int* off,
                             const int* cnt, int ncnt, int samples_per_row, double* acc, hipStream_t st);
void fwn_launch_ragged_finish(const float* planes, long nclip, long T, const double* acc, int nflows, int n_flow, const int* len,
                              float* out2B, hipStream_t st);
// windowed forward (aux_kernels.hip; fwn.h has the contracts).  fwn_launch_window_sums: window c's partial sums (z^2 over its
// core of the final planes [2][n][L / 2], -log_s and the ActNorm terms over acc [nflows][n][nslot] - fwn_launch_range_logdet's
// over the core's rows -, the core's length) -> out[slot[c]][0 .. 4) fp64.  fwn_launch_window_latent: the cores of the planes in
// time order -> z + out_off[c] (swapped: n_block * n_flow is odd).  fwn_launch_windows_finish: per clip, its windows' sums
// part[slot0[c] .. slot0[c] + nwin[c])[4] in window order -> out2B [2][nclip].  Every table is read and clamped on the device.
void fwn_launch_window_sums(const float* planes, long n, long L, const int* core_off, const int* core_len, const double* acc,
                            int nflows, int n_flow, const int* slot, double* out, hipStream_t st);
void fwn_launch_window_latent(const float* planes, long n, long L, int swapped, const int* core_off, const int* core_len,
                              const long long* out_off, float* z, hipStream_t st);
void fwn_launch_windows_finish(const double* part, const int* slot0, const int* nwin, long nclip, float* out2B, hipStream_t st);
void fwn_launch_ddi(const float* xa, const float* xb, int M, int Ch, float* an, hipStream_t st);
void fwn_launch_ddi_moments(const float* xa, const float* xb, int M, int Ch, double* mom, hipStream_t st);
void fwn_launch_ddi_from_moments(const double* mom, int Ch, float* an, hipStream_t st);
// ragged ActNorm init (aux_kernels.hip): fwn_launch_ddi_moments over rows [0, len[c] / samples_per_row) of every clip c of
// [nclip][rows][Ch] planes, mom[4 Ch] = the rows counted.  part: [fwn_ragged_moments_nslot(nclip, rows, Ch)][4 Ch] fp64 scratch.
int fwn_ragged_moments_nslot(long nclip, long rows, int Ch);
void fwn_launch_ddi_moments_ragged(const float* xa, const float* xb, long nclip, long rows, int Ch, const int* len,
                                   int samples_per_row, double* mom, double* part, hipStream_t st);
void fwn_launch_prior(const float* planes, long n, const float* partial, int n_partial, double inv_bt,
                      float* out2, hipStream_t st);

int fwn_sqnorm_blocks(long n);
void fwn_launch_mel(const float* wav, long B, long T, const float* window, const float* fb, int n_fft, int hop,
                    int n_mels, float ref_db, float min_db, float* mel, hipStream_t st);
void fwn_launch_grad_norm(const float* g, long n, float gscale, double* partial, float* out, hipStream_t st);
void fwn_launch_adam(float* w, const float* g, float* m, float* v, long n, const float* gnorm, float gscale,
                     float clip, float lr_t, const float* lr_dev, float b1, float b2, float eps, hipStream_t st);
// dst[i] = a ? a[i] + b[i] : b[i]; dst may be a or b.  float4 body when the pointers share one misalignment mod 16, else dwords
void fwn_launch_grad_accumulate(float* dst, const float* a, const float* b, long n, hipStream_t st);

// train_kernels.hip
struct fwn_gemm_desc;
int fwn_gemm_launch(const fwn_gemm_desc* g, hipStream_t st);
int fwn_gemm_tile_rule(const fwn_gemm_desc* g);      // BM * 1000 + BN of the tile fwn_gemm_launch runs
void fwn_transpose_launch(const void* src, int M, int C, int ld_src, int shift0, int dshift, int ntap, int Ti, void* dst,
                          int ld_dst, int ones_row, hipStream_t st);
void fwn_reduce_splits_launch(const float* partial, int nsplit, long stride, long n, float scale, float* out,
                              hipStream_t st);
void fwn_ew_actnorm_fwd(float* x, const float* an, long n, int Ch, hipStream_t st);
void fwn_ew_actnorm_fwd2(float* xa, float* xb, const float* an2, long n, int Ch, hipStream_t st);
void fwn_ew_coupling_fwd(float* yb, const float* Z, const float* ez, long n, int Ch, float* partial, int nblocks,
                         hipStream_t st);
void fwn_ew_coupling_bwd(float* g, float* ob, const float* Z, const float* ez, long n, int Ch, float cls, void* dZ,
                         int ldz, float* dzz, hipStream_t st);
void fwn_ew_coupling_bwd_ex(float* g, float* ob, const float* Z, const float* ez, long n, int Ch, float cls, void* dZ,
                            int ldz, float* dzz, const float* ya, void* ya_bf, int ldya, hipStream_t st);
// ragged batch (nclip clips of `rows` rows, clip b keeps len[b] / spr): per-clip log-det term, zeros past a clip's end
void fwn_ew_coupling_bwd_ragged(float* g, float* ob, const float* Z, const float* ez, long nclip, long rows, int Ch, const int* len,
                                int spr, void* dZ, int ldz, float* dzz, const float* ya, void* ya_bf, int ldya, hipStream_t st);
void fwn_ew_gate_bwd(const void* do_, int ld_do, const void* aux, long n, void* dpre, hipStream_t st);
int fwn_colsum_blocks(long M, int C);
void fwn_ew_colsum_prod(const float* A, const float* B, long M, int C, float scale, float* partial, float* out,
                        hipStream_t st);
void fwn_ew_actnorm_bwd(float* dy, float* y, const float* an, long n, int Ch, hipStream_t st);
int fwn_small_grads_blocks(long M, int Ch);
void fwn_small_grads_main(float* ga, float* ya, float* gb, float* yb, const float* dzz, const float* an, long M, int Ch,
                          double* partial, hipStream_t st);
void fwn_small_grads_main_ragged(float* ga, float* ya, float* gb, float* yb, const float* dzz, const float* an, long nclip, long rows,
                                 int Ch, const int* len, int spr, double* partial, hipStream_t st);
void fwn_small_grads_final(const float* an, long M, int Ch, const long long* br, const long long* zc, const double* partial, float* db,
                           float* dlogs, float* dzscale, hipStream_t st);
void fwn_small_grads_launch(float* ga, float* ya, float* gb, float* yb, const float* dzz, const float* an, long M, int Ch,
                            const long long* br, const long long* zc, double* partial, float* db, float* dlogs,
                            float* dzscale, hipStream_t st);
struct fwn_wn_job;
struct fwn_tn_job;
long fwn_wn_group_scratch_doubles(const fwn_wn_job* jobs, int njobs);
void fwn_wn_group_launch(const fwn_wn_job* jobs, int njobs, double* scratch, hipStream_t st);
int fwn_up_bwd_chunks(int B, int H);
void fwn_up_bwd_launch(float* dy, const float* y, const float* x, int B, int H, int W, int s, const float* wk,
                       float* dx, float* dwk_bias, float* partial, hipStream_t st);
struct fwn_scale_job;
struct fwn_pack_job;
void fwn_launch_pack_jobs(const fwn_scale_job* sjobs, int nsjobs, const fwn_pack_job* jobs, int njobs, float* scales,
                          int scale_ld, hipStream_t st);
int fwn_tn_tile(int M);
void fwn_tn_group_launch(const fwn_tn_job* jobs, int njobs, int M, int Ti, hipStream_t st);
size_t fwn_tn_table_bytes(void);
int fwn_tn_multi_max(void);
void fwn_tn_multi_launch(const fwn_tn_job* const* jobs, const int* njobs, int ngroups, int M, int Ti, void* table, hipStream_t st);
void fwn_colsum_bf16_launch(const void* dy, long M, int C, int ld, float scale, float* partial, float* out, hipStream_t st);
