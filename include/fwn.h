/*
 * fwn.h - C ABI of libfwn.so: the MI355X (gfx950) FloWaveNet flow forward / inverse path.
 *
 * The reference (ryhorv/tf-flowavenet) has no FFI seam: its hot path sits behind the Python
 * class FloWaveNet (model.py:282-404) whose arithmetic is delegated to TensorFlow 1.12 ops.
 * This header is the boundary a maintainer binds instead of those TF ops (ctypes stub in
 * INTEGRATION.md).  Conventions:
 *   - every pointer is a DEVICE pointer into caller-owned memory unless marked "host";
 *   - sizes are explicit, the HIP stream is the last argument (void*, may be NULL = default);
 *   - no allocation, no synchronisation, no hidden global state: calls are asynchronous on
 *     `stream` and safe to issue concurrently on distinct streams with distinct workspaces;
 *   - return 0 on success, <0 on error; fwn_last_error() returns a thread-local message.
 *
 * Device data layouts (DESIGN.md "Data layout in HBM"):
 *   flow state   : fp32 planes[2][B][T/2]; plane q holds samples 2s+q.  At block i a plane is the
 *                  row-major matrix [M = B*T_i][Ch = 2^i], T_i = T / 2^(i+1).  The reference's
 *                  squeeze / unsqueeze (model.py:226-239,260-273) and change_order (:166-174)
 *                  are index bookkeeping on these planes: no data moves.
 *   conditioning : bf16 cplanes[2][B][T][num_mels/2]; plane q holds mel bins [q*half, (q+1)*half).
 *   hidden       : bf16 [M][256].
 *   weights      : bf16, weight-norm folded, [N][K] with K contiguous, permuted to the plane
 *                  orders above (tf-flowavenet_amd/packing.py builds the index tables).
 */
#ifndef FWN_H
#define FWN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FWN_VERSION 322            /* (round 7, number kept: + fwn_flow_desc.Wds appended and fwn_gate_tile; fwn_flow_desc grew, so a host that builds
                                    * the flows array must be rebuilt against this header.)  0.3.22: - fwn_train_desc.an_logdet and .defer_block_done (a host built against 0.3.21 must be rebuilt).
                                    * 0.3.21 (round 6): + fwn_model_desc.cond_stream (appended) and fwn_cond_stream* / fwn_pack_cond_stream (the register-streamed
                                    * conditioning projection, csrc/cond_rs.h; additive); fwn_pack_tail_stream_jobs.  0.3.20 (round 6): + fwn_flow_desc.Wts and fwn_tail_stream_bytes / fwn_pack_tail_stream / fwn_tail_stream_rows (the
                                    * register-streamed tail, csrc/tail_rs.h; additive: a 0.3.10 host that zero-fills its descriptors keeps working);
                                    * fwn_tail_partials / fwn_tail_partials_chained are upper bounds now.  0.3.10 (round 5): + fwn_flow_run_persist / fwn_flow_persist_* (one launch per small-M flow), fwn_model_desc.persist_mode
                                    * (was `reserved`: 0 keeps working), fwn_set_option.  0.3.1: + fwn_gate_clock (additive: a 0.3.0 host keeps working).  0.3.0: fwn_flow_desc gained Wfront3 / kf3 (round 3) and Wgs (round 4), fwn_model_desc
                                    * chain_mode, fwn_block_done_fn returns int; Wskip / Wfinal rows and biases are in
                                    * acc_k_perm order, Wzero's K axis is natural.  A host built against 0.2.0 must be
                                    * rebuilt and repack its weights. */
#define FWN_MAX_LAYERS 8
#define FWN_MAX_UPSAMPLE 4

#define FWN_OK 0
#define FWN_ERR_ARG (-1)           /* bad argument (null pointer, size, alignment, config) */
#define FWN_ERR_HIP (-2)           /* a HIP launch or runtime call failed */
#define FWN_ERR_WORKSPACE (-3)     /* workspace too small */
#define FWN_ERR_CALLBACK (-4)      /* a host callback (fwn_block_done_fn) asked to stop */

int fwn_version(void);
const char* fwn_last_error(void);

/* ---- K10: weight-norm + bf16 packing (replaces convolutional.py:73-80 + utils.py:19-29) ----
 * v is the TF-layout kernel flattened to [k_src][n_src] (k_src = kernel_size*C_in, n fastest).
 * scale[n] = g[n] / sqrt(max(sum_k v[k][n]^2, 1e-12)). */
int fwn_wn_scale(const float* v, const float* g, int k_src, int n_src, float* scale, void* stream);
/* out[n'*ld_dst + k'] = bf16(v[src_k[k']][src_n[n']] * scale[src_n[n']]) for n' < n_dst, k' < k_dst.
 * src_k[k'] < 0 writes 0 (K padding); rows with src_n[n'] < 0 are left untouched; scale may be NULL. */
int fwn_pack_bf16(const float* v, const float* scale, const int32_t* src_k, const int32_t* src_n,
                  int n_src, int k_dst, int n_dst, int64_t ld_dst, void* out_bf16, void* stream);

/* Grouped form: a whole model's scales and packed copies in two launches.  Both job tables live in
 * device memory; scale job s writes scales[s][0..n_src) (g / ||V||_col), pack job p multiplies by
 * scales[p.scale_slot] (slot < 0: none) and by p.mul; transposed: out[k][n] (ld_dst >= n_dst)
 * instead of out[n][k].  Index tables as in fwn_pack_bf16. */
typedef struct fwn_scale_job { const float* v; const float* g; int32_t k_src, n_src; } fwn_scale_job;
typedef struct fwn_pack_job {
    const float* v; const int32_t* src_k; const int32_t* src_n; void* out; int64_t ld_dst;
    int32_t n_src, k_dst, n_dst, scale_slot, transposed; float mul;
} fwn_pack_job;
int fwn_pack_jobs(const fwn_scale_job* scale_jobs, int n_scale_jobs, const fwn_pack_job* pack_jobs, int n_pack_jobs,
                  float* scales, int scale_ld, void* stream);

/* ---- small fp32 parameter tables straight from a flat vector of fp32 masters (a training step refreshes biases,
 * ActNorm / ZeroConv tables and the up-sampling kernels on the device, inside its hipGraph):
 * fwn_gather_tables: out[i] = F(post[i] * sum_t flat[idx[t*total + i]]) for i < total (idx < 0: term absent);
 *                    mode[i] 0: identity, 1: exp, both in fp64 rounded once; 2 / 3: the same in fp32, terms in order
 * fwn_sum_f32      : out[0] = sum_i in[i] (fixed order, fp64 accumulation)
 * fwn_upsample_wn  : the weight-normed up-sampling kernel out[2s][3] = v / ||v||_(k per kw column) * g (convolutional.py:179-186) */
int fwn_gather_tables(const float* flat, const int64_t* idx, int nterm, int64_t total, const double* post,
                      const unsigned char* mode, float* out, void* stream);
int fwn_sum_f32(const float* in, int64_t n, float* out, void* stream);
int fwn_upsample_wn(const float* v, const float* g, int s, float* out, void* stream);

/* ---- K1: one upsampling stage (replaces Conv2DTranspose.call + leaky_relu, model.py:301-311,
 * 398-404).  in [B][H][W] fp32, wk = weight-normed kernel [2s][3] fp32 (device), out rows H*s.
 * Exactly one of out_f32 ([B][H*s][W]) / out_cplanes (bf16 [2][B][H*s][W/2]) may be NULL. */
int fwn_upsample_stage(const float* in, int B, int H, int W, const float* wk, float bias, int s,
                       float* out_f32, void* out_cplanes, void* stream);
/* The same stage with the bias read from device memory (one float, e.g. the fp32 master itself): the launch
 * carries no parameter value and can be replayed from a hipGraph after the parameter changed. */
int fwn_upsample_stage_dev(const float* in, int B, int H, int W, const float* wk, const float* bias, int s,
                           float* out_f32, void* out_cplanes, void* stream);

/* ---- K2: x[B][T] <-> planes[2][B][T/2] (squeeze / unsqueeze entry and exit) ---- */
int fwn_split_planes(const float* x, int64_t B, int64_t T, float* planes, void* stream);
int fwn_merge_planes(const float* planes, int64_t B, int64_t T, float* x, void* stream);

/* ---- K3 (init only): ActNorm data-dependent init of one flow (model.py:30-83).
 * an[2][4][Ch] <- per (a|b) plane: shift b, scale exp(3 logs), inverse scale, 3*logs. */
int fwn_actnorm_ddi(const float* xa, const float* xb, int M, int Ch, float* an, void* stream);
/* The same init for a batch sharded over ranks (the reference's towers race on this assign, model.py:39 under
 * train.py:43-57): fwn_actnorm_moments writes this rank's mom[4 Ch + 1] doubles = per plane (sum_m x | sum_m x^2)
 * [2][2][Ch] followed by the row count M; the caller all-reduces (sums) them over the ranks;
 * fwn_actnorm_from_moments turns the global moments into the table `an` - identical on every rank. */
int fwn_actnorm_moments(const float* xa, const float* xb, int M, int Ch, double* mom, void* stream);
int fwn_actnorm_from_moments(const double* mom, int Ch, float* an, void* stream);

/* Static description of one flow (model.py:176-205 Flow = ActNorm + AffineCoupling(WaveNet)).
 * All pointers are device pointers to packed weights; layouts in packing.py. */
typedef struct fwn_flow_desc {
    int32_t Ch;          /* channels per plane at this block = 2^i */
    int32_t cin;         /* conditioning channels of c_a = (num_mels/2) * 2^(i+1) */
    int32_t kcpad;       /* cin rounded up to 64 */
    int32_t kfpad;       /* 3*Ch rounded up to 64 */
    int32_t npt;         /* ZeroConv pair tiles = max(1, ceil(Ch/32)) */
    int32_t L;           /* n_layer */
    const void* Wfront;  const float* bfront;               /* [256][kfpad], [256]            */
    const void* Wfront2;                                    /* Ch >= 32: [256][6*Ch], K = tap*2Ch + (hi|lo)*Ch + tau; Ch = 16: the same
                                                               with 32 channels per half, tau >= 16 zero ([256][192]); else NULL */
    /* Gate operands are stored pre-multiplied by the exponent scale of their nonlinearity: filter
     * rows by -2*log2(e), gate rows by -log2(e) (tanh(f)*sigmoid(g) from two exp2, packing.py GATE_MUL). */
    const void* Wd[FWN_MAX_LAYERS];                         /* [512][768] gate-packed rows     */
    const void* Wc[FWN_MAX_LAYERS];                         /* [512][kcpad]                    */
    const float* bgate[FWN_MAX_LAYERS];                     /* [512] conv bias + cond bias     */
    const void* Wres[FWN_MAX_LAYERS];                       /* [256][256] (layers 0..L-2)      */
    const float* bres[FWN_MAX_LAYERS];
    /* Wskip / Wfinal: row n' holds output channel n' with bits 2 and 3 swapped (packing.acc_k_perm: the order the tail
     * kernel's accumulator registers feed the next MFMA chain in), biases alike; every K axis in natural channel order */
    const void* Wskip;   const float* bskip;                /* [256][L*256], [256] (sum)       */
    const void* Wfinal;  const float* bfinal;               /* [256][256], [256]               */
    const void* Wzero;   const float* bzero; const float* ezero;   /* [npt*64][256], [npt*64]x2 */
    float* an;                                              /* [2][4][Ch] ActNorm (DDI writes)  */
    /* fp8 dilated-conv path (BASELINE configs[4]); NULL = not packed.  Wd8[l]: the gate-packed rows of Wd[l] as OCP
     * e4m3 bytes [512][768], stored as W * 2^wd8_exp[l] (one power-of-two scale per matrix, fwn_pack_e4m3). */
    const void* Wd8[FWN_MAX_LAYERS];
    int32_t wd8_exp[FWN_MAX_LAYERS];
    /* Chained front conv (Ch <= 8, else NULL / 0): the front weights once more as [256][kf3], K = (tap*Ch + tau)*2 + (hi|lo),
     * kf3 = 6*Ch rounded up to 16.  With it the whole-model calls let the tail of the PREVIOUS flow of the block compute
     * this flow's h0 (csrc/tail_chain.h); the stage entry points ignore it. */
    const void* Wfront3;
    int32_t kf3, reserved;
    /* Register-streamed gate (csrc/gate_rs.h; NULL = not packed): Wd[l] and Wc[l] once more in MFMA-fragment order
     * (fwn_pack_gate_stream), read by the gate kernel of the largest row counts (fwn_gate_stream_rows) instead of them. */
    const void* Wgs[FWN_MAX_LAYERS];
    /* Register-streamed tail (csrc/tail_rs.h; NULL = not packed): Wskip | Wfinal once more in MFMA-fragment order
     * (fwn_pack_tail_stream), read by the tail kernel of the larger row counts (fwn_tail_stream_rows) instead of them. */
    const void* Wts;
    /* Register-streamed hoisted gate (round 7, csrc/cond_rs.h gate_hs_kernel; NULL = not packed): Wd[l] alone in the fragment
     * order of the conditioning stream - fwn_pack_cond_stream(Wd[l], 512 * 768, 768, 1, out), fwn_cond_stream_bytes(768) bytes -
     * read instead of Wd[l] by the gates with a hoisted P whose rows the ring path would give its un-split 64 x 128 tile
     * (3 009 - 6 016 rows, dilation <= 3).  Bit-identical to that path.  Appended: the descriptor grew by 8 * FWN_MAX_LAYERS
     * bytes, a host must be rebuilt against this header (the flows of a model are an array of these). */
    const void* Wds[FWN_MAX_LAYERS];
} fwn_flow_desc;

/* ---- fragment-order tail weights (round 6, csrc/tail_rs.h; replaces nothing in the reference: a second packing of the
 * operands of modules.py:175-179 for the kernel that streams them to registers).
 * fwn_tail_stream_bytes: size of the stream of one flow with L layers, 0 if no kernel is built for that L (L = 2 only);
 * fwn_pack_tail_stream : Wskip [256][L*256], Wfinal [256][256] (rows in accumulator order, as in fwn_flow_desc) -> out;
 * fwn_tail_stream_rows : smallest M from which fwn_tail / fwn_tail_chained / fwn_tail_train and the flow and model calls
 *                        use the stream (one ZeroConv pair tile: Ch <= 32). */
int64_t fwn_tail_stream_bytes(int L);
int fwn_pack_tail_stream(const void* Wskip, const void* Wfinal, int L, void* out, void* stream);
/* The same for njobs flows in one launch: `jobs` is a DEVICE array of {Wskip, Wfinal, out} device pointers (a training step
 * re-packs every flow's stream behind its grouped weight packing: packing.PackPlan). */
typedef struct fwn_tail_stream_job { const void* Wskip; const void* Wfinal; void* out; } fwn_tail_stream_job;
int fwn_pack_tail_stream_jobs(const fwn_tail_stream_job* jobs, int njobs, int L, void* stream);
int fwn_tail_stream_rows(void);

/* ---- fragment-order gate weights (round 4, csrc/gate_rs.h; replaces nothing in the reference: a second packing of the
 * operands of modules.py:113-124 for the kernel that streams them to registers).
 * fwn_gate_stream_bytes: size of the stream for `cin` conditioning channels, 0 if no kernel is built for that cin;
 * fwn_pack_gate_stream : Wd [512][768], Wc [512][kcpad] (gate-packed rows, as in fwn_flow_desc) -> out;
 * fwn_gate_stream_rows : smallest M from which fwn_gate / the flow and model calls use the stream (dilation <= 3,
 *                        Ti >= 256, conditioning fused: ca given, no training aux). */
int64_t fwn_gate_stream_bytes(int cin);
int fwn_pack_gate_stream(const void* Wd, const void* Wc, int cin, int kcpad, void* out, void* stream);
int fwn_gate_stream_rows(void);
/* Diagnostic (bench.py's roofline.clock_ghz): ONE launch of the register-streamed gate of `layer` exactly as fwn_gate would
 * run it at this shape (256-row tiles: M >= 24 576 rows, Wgs set), from an instantiation that also stamps the shader clock
 * (s_memtime) and the 100 MHz reference (s_memrealtime) at the start and end of every wave:
 * stamps[(workgroup * 8 + wave) * 4 + {0, 1, 2, 3}] = {cycles at start, at end, reference at start, at end}; returns the
 * number of workgroups (stamps holds 32 * that many uint64_t) or a negative error code if the shape has no such kernel.
 * In-kernel clock of a wave = (s[1] - s[0]) / (s[3] - s[2]) x 100 MHz; take it after seconds of back-to-back launches. */
int fwn_gate_clock(const fwn_flow_desc* d, int layer, const void* h, const void* ca, void* o, int M, int Ti, uint64_t* stamps,
                   void* stream);

/* ---- stage entry points (K4..K8), exposed so each kernel can be parity-tested alone ---- */
/* K4 front conv k=3 + ReLU over in_a (modules.py:144,164-165); apply_an: ActNorm on load.
 * scratch: NULL or [M][256] bf16 (for Ch >= 32 the fp32 state is first laid out as a hi|lo bf16
 * matrix there so the conv runs on the LDS-DMA ring GEMM; fwn_flow_run lends its second h buffer). */
int fwn_front(const fwn_flow_desc* d, const float* xa, void* h_out, void* scratch, int M, int Ti, int apply_an,
              void* stream);
/* K5 gated dilated layer `layer` (modules.py:113-124).  ca==NULL uses P (precomputed c_a@Wc). */
int fwn_gate(const fwn_flow_desc* d, int layer, const void* h, const void* ca, const float* P, void* o,
             int M, int Ti, void* stream);
/* K5 with a hoisted P on ONE named tile (tests and tile sweeps; every tile gives fwn_gate's bits): cols = 512 | 256 with
 * rows = 64 | 96 | 128: the register-streamed form from d->Wds[layer] (rows = cols = 0: the tile fwn_gate takes), only at the
 * shapes where fwn_gate would take it; cols = 128 with rows = 64 | 128 | 256: the ring tile of that height from d->Wd[layer].
 * Returns the number of workgroups launched or a negative error code. */
int fwn_gate_tile(const fwn_flow_desc* d, int layer, const void* h, const float* P, void* o, int M, int Ti, int rows, int cols,
                  void* stream);
/* K5 with the dilated taps in fp8 (v_mfma_scale_f32_32x32x64_f8f6f4): h8 = e4m3 copy of h [M][256] bytes
 * (fwn_cast_e4m3, or written by the front / res kernels inside fwn_flow_run_fp8), weights d->Wd8[layer]; the 1x1
 * conditioning conv stays bf16 in the same accumulators.  Exists for the MFMA-bound shapes only:
 * fwn_gate_fp8_supported(M, layer) != 0 (M >= 12288 rows, dilation <= 3); other shapes return FWN_ERR_ARG. */
int fwn_gate_fp8_supported(int M, int layer);
int fwn_gate_fp8(const fwn_flow_desc* d, int layer, const void* h8, const void* ca, void* o, int M, int Ti, void* stream);
/* bf16 [n] -> OCP e4m3 [n] (round to nearest even, saturating at +-448). */
int fwn_cast_e4m3(const void* src_bf16, void* dst_u8, int64_t n, void* stream);
/* e4m3 weight packing: fwn_wn_absmax folds max |v[k][n] scale[n] mul| of one source kernel into *amax (a device
 * float, zero it first; scale may be NULL); fwn_pack_e4m3 then writes out[n'*ld_dst + k'] = e4m3(v[src_k[k']][src_n[n']]
 * scale mul 2^e) with e = floor(log2(448 / *amax)) and stores e in *exp_out (device int32).  Index tables as in
 * fwn_pack_bf16 (several source kernels may share one output matrix and one amax: filter and gate rows). */
int fwn_wn_absmax(const float* v, const float* scale, int k_src, int n_src, float mul, float* amax, void* stream);
int fwn_pack_e4m3(const float* v, const float* scale, const int32_t* src_k, const int32_t* src_n, int n_src, int k_dst,
                  int n_dst, int64_t ld_dst, float mul, const float* amax, void* out_u8, int32_t* exp_out, void* stream);
/* K6 residual 1x1 (modules.py:126-128): h_out = (h_in + res_conv(o)) * sqrt(0.5). */
int fwn_res(const fwn_flow_desc* d, int layer, const void* o, const void* h_in, void* h_out, int M,
            void* stream);
/* K5' conditioning projections of a parity group of flows in one launch: for j = flow0, flow0 +
 * flow_step, ... (nflow flows) and every layer: P[j*L+l] = ca @ Wc[j][l].  Wc_base/w_stride address
 * the block-contiguous weights, P_base/p_stride the outputs ([M][512] fp32 each). */
int fwn_cond(const void* ca, const void* Wc_base, float* P_base, int64_t w_stride, int64_t p_stride,
             int flow0, int flow_step, int nflow, int L, int M, int cin, int kcpad, void* stream);
/* The same with the K range dealt over nsplit workgroups per tile (few rows against a long K: M = 63 rows, cin = 10240
 * at the last block of a single clip): split 0 writes P, split z > 0 the same matrices into part + (z - 1) part_stride
 * (floats; laid out like P); fwn_cond_reduce then adds the partials to P[0..n) in ascending order (bit-reproducible).
 * fwn_cond_splits: the split count the model-level calls use for nz = nflow * L matrices per launch (1: none). */
int fwn_cond_splits(int M, int nz, int kcpad);
int fwn_cond_split(const void* ca, const void* Wc_base, float* P_base, int64_t w_stride, int64_t p_stride,
                   int flow0, int flow_step, int nflow, int L, int M, int cin, int kcpad, float* part, int64_t part_stride,
                   int nsplit, void* stream);
int fwn_cond_reduce(float* P, const float* part, int64_t part_stride, int nsplit, int64_t n, void* stream);
/* ---- fragment-order conditioning weights (round 6, csrc/cond_rs.h; replaces nothing in the reference: a second packing of the
 * same [512][kcpad] matrices) for the hoisted projection from fwn_cond_stream_rows() rows on: a workgroup = 128 rows x one whole
 * matrix, weights streamed to registers, activations staged once in LDS (63 GFLOP of block 4 - 7 of the 8-clip pass in 55 - 65 us
 * against 76 - 93 for the ring tiles).
 * fwn_cond_stream_bytes : size of ONE matrix's stream (= the matrix: 512 kcpad 2 bytes), 0 if kcpad is not a multiple of 64
 * fwn_pack_cond_stream  : nz matrices Wc_base + z w_stride ([512][kcpad] bf16 each) -> out (nz streams back to back)
 * fwn_cond_stream       : P[j L + l] = ca @ Wc[j][l] for the nflow flows and L layers of a block in one launch (flows with an odd
 *                         index read ca_odd if given); nsplit > 1: like fwn_cond_split, then fwn_cond_reduce
 * fwn_cond_stream_splits: the split count the model-level calls use */
int64_t fwn_cond_stream_bytes(int kcpad);
int fwn_cond_stream_rows(void);
int fwn_cond_stream_splits(int M, int nz, int kcpad);
int fwn_pack_cond_stream(const void* Wc_base, int64_t w_stride, int kcpad, int nz, void* out, void* stream);
int fwn_cond_stream(const void* ca, const void* ca_odd, const void* Ws, float* P, int nflow, int L, int M, int cin, int kcpad,
                    float* part, int64_t part_stride, int nsplit, void* stream);
/* K6'+K7+K8 tail: skip sum, final 1x1, ZeroConv1d, affine coupling, ActNorm, log-det partials
 * (modules.py:175-180,51-56; model.py:86-102,124-141,146-161).  o = [L][M][256].
 * partial (forward only, may be NULL) receives AT MOST fwn_tail_partials(M) partial sums (how many depends on the kernel
 * that serves the flow's packed operands at this M: zero the buffer first, its sum is the log-det).
 * Large M: one register-chained kernel.  M <= 12288 rows: three GEMM launches whose weights are split over the
 * workgroups by output column (a workgroup of the fused kernel streams all 0.4 - 0.5 MB of tail weights itself:
 * 22 - 36 us whatever the row count); they keep S and U in `scratch` = [2][M][256] bf16 (may be NULL for larger M). */
int fwn_tail_partials(int M);
/* The exact count for flow d at M rows (which kernel serves it depends on its packed operands: d->Wts): mode -1 = fwn_tail /
 * fwn_tail_train, 0 = fwn_tail_chained without a next flow, 1 = with one.  Always <= the bounds above. */
int fwn_tail_partials_desc(const fwn_flow_desc* d, int M, int mode);
int fwn_tail(const fwn_flow_desc* d, const void* o, float* xa, float* xb, float* partial, int M,
             int inverse, void* scratch, void* stream);
/* The tail as the whole-model calls chain it (csrc/tail_chain.h), exposed for stage-level parity tests: out_b goes to
 * xb_out (a third plane buffer: xb is left untouched) and, when `next` is given (the flow that runs after d: Ch <= 8,
 * next->Wfront3 packed), next's front conv + ReLU (modules.py:144,164-165; forward: behind next's ActNorm) is computed in
 * the same launch into h0_next [M][256] bf16.  partial (forward) receives fwn_tail_partials_chained(M, d->Ch, next != NULL)
 * sums.  scratch as in fwn_tail.  Returns FWN_ERR_ARG where the tail at this shape cannot chain (fwn_tail_can_chain). */
int fwn_tail_can_chain(const fwn_flow_desc* d, int M, int with_front);
int fwn_tail_partials_chained(int M, int Ch, int with_front);
int fwn_tail_chained(const fwn_flow_desc* d, const fwn_flow_desc* next, const void* o, float* xa, const float* xb, float* xb_out,
                     void* h0_next, float* partial, int M, int Ti, int inverse, void* scratch, void* stream);
/* The same tail as the training step runs it (forward direction): it also keeps what the backward needs -
 * save_s = S = ReLU(skip sum) and save_u = U = ReLU(final conv), bf16 [M][256] in natural channel order, and
 * save_z = Z = U Wz + bz, fp32 [M][2 Ch] (log_s channels then t channels, plane order; before the exp(3 scale) factor).
 * o: layer l at o + l * o_stride elements (the training step keeps every layer's output in a buffer of its own). */
int fwn_tail_train(const fwn_flow_desc* d, const void* o, int64_t o_stride, float* xa, float* xb, float* partial, int M,
                   void* save_s, void* save_u, float* save_z, void* stream);

/* ---- one whole flow (replaces Flow.forward / Flow.reverse, model.py:185-202) ----
 * xa / xb: the planes holding in_a / in_b for this flow's swap parity, ca the matching
 * conditioning plane.  h0/h1: [M][256] bf16 scratch, o: [L][M][256] bf16 scratch,
 * P: NULL or [L][M][512] fp32 precomputed conditioning projections for this flow,
 * partial: NULL or [fwn_tail_partials(M)] log-det partial sums (forward).  ddi: run fwn_actnorm_ddi first. */
int fwn_flow_run(const fwn_flow_desc* d, int64_t B, int64_t T, float* xa, float* xb, const void* ca,
                 void* h0, void* h1, void* o, const float* P, float* partial, int inverse, int ddi,
                 void* stream);

/* ---- one whole flow as ONE launch (round 5, csrc/flow_persist.h): the same arithmetic as fwn_flow_run, bit for bit, for the
 * shapes where every stage of the flow is a launch of a handful of workgroups (the dependent-launch floor of the small
 * blocks: model.py:394-396 run one utterance at a time, synthesize.py:40-49).  Tickets (stage, 64-row tile, 64-column
 * tile) are taken from an atomic counter by 8-wave workgroups, dependencies are per row tile, a ticket's weights are
 * requested before it waits for its producers; hand-offs are write-through stores + agent-scope counters + sc1 loads.
 * Preconditions (fwn_flow_persist_supported != 0): conditioning hoisted (P given, ca == NULL), n_layer <= 2,
 * M = B * T / (2 Ch) <= 4096 rows, forward or inverse without data-dependent init, bf16 gates.
 * sync: fwn_flow_persist_sync_bytes(M, L) bytes of device memory that the CALLER ZEROES (stream-ordered) before every call;
 * sync[1] != 0 afterwards = a bounded spin gave up (fwn_flow_persist_status reads it back: that one synchronises); the flow's
 * outputs are then NaN (plane elements and log-det partials of the row tiles down the chain), also inside the whole-model
 * calls: log_p / logdet / the waveform come back NaN, never silently wrong. */
int fwn_flow_persist_supported(const fwn_flow_desc* d, int64_t B, int64_t T);
int64_t fwn_flow_persist_sync_bytes(int M, int L);
int fwn_flow_run_persist(const fwn_flow_desc* d, int64_t B, int64_t T, float* xa, float* xb, void* h0, void* h1, void* o,
                         const float* P, float* partial, int inverse, void* sync, void* stream);
int fwn_flow_persist_status(const void* sync, void* stream);
/* ---- process-wide developer options (replaces the environment variables the launch path read in round 4) ----
 * name: "rs_persist" (-1 auto, 0 / 1: the register-streamed gate's persistent form off / on); "persist_spin_us" (bound of the
 * one-launch flow's dependency spins in microseconds, 0 = the default 2 s: tests shorten it to provoke a give-up).  Returns the previous value,
 * or FWN_ERR_ARG for an unknown name.  (Round 4's second switch, the experimental co-resident gate, left the library:
 * tools/gate_co.h + tools/bench_gate_co.hip.) */
int fwn_set_option(const char* name, int value);

/* The same flow with the gated layers' dilated taps in fp8 wherever fwn_gate_fp8_supported says so (other layers /
 * shapes run the bf16 kernels): h8a / h8b are [M][256]-byte scratch buffers for the e4m3 copies of h. */
int fwn_flow_run_fp8(const fwn_flow_desc* d, int64_t B, int64_t T, float* xa, float* xb, const void* ca,
                     void* h0, void* h1, void* o, const float* P, float* partial, int inverse, int ddi,
                     void* h8a, void* h8b, void* stream);

/* ---- mel front-end (preprocessing.py:58-69; librosa.feature.melspectrogram semantics) ----
 * wav [B][T] fp32 -> mel [B][1 + T/hop][n_mels] in [0, 1]: centred STFT (reflect padding, `window`
 * [n_fft], power 2), `fb` [n_mels][n_fft/2 + 1] filterbank, 20 log10(max(1e-4, .)) - ref_level_db,
 * then clip((. - min_level_db) / -min_level_db, 0, 1).  n_fft a power of two, T > n_fft / 2. */
int fwn_mel_spectrogram(const float* wav, int64_t B, int64_t T, const float* window, const float* fb, int n_fft,
                        int hop, int n_mels, float ref_level_db, float min_level_db, float* mel, void* stream);

/* ---- K9: prior + log-det finalisation (model.py:342-347) ----
 * out2[0] = mean(0.5(-log 2pi - z^2)) over n = B*T plane elements, out2[1] = sum(partial)/(B*T). */
int fwn_prior_logp(const float* planes, int64_t n, const float* partial, int n_partial, float* out2,
                   void* stream);

/* ---- data-parallel optimiser step (replaces average_gradients + un-scale + clip_by_global_norm
 * + AdamOptimizer.apply_gradients, utils.py:34-60, train.py:27-32,75-81).  g is the flat fp32
 * gradient buffer AFTER the RCCL all-reduce (a sum over ranks); gscale = 1/(world * loss_scale)
 * turns it into the reference's averaged, un-scaled gradient.
 * fwn_grad_norm: gnorm_out[0] = ||g * gscale||_2 (deterministic; partial holds
 * fwn_grad_norm_partials(n) doubles).  fwn_clip_adam: g' = g*gscale * clip / max(gnorm, clip),
 * then TF-form Adam (lr_t = lr*sqrt(1-b2^t)/(1-b1^t), eps outside the sqrt) on fp32 masters. */
int fwn_grad_norm_partials(int64_t n);
int fwn_grad_norm(const float* g, int64_t n, float gscale, double* partial, float* gnorm_out, void* stream);
int fwn_clip_adam(float* w, const float* g, float* m, float* v, int64_t n, const float* gnorm, float gscale,
                  float clip, float lr, int64_t step, float beta1, float beta2, float eps, void* stream);
/* The same update with the bias-corrected rate lr_t = fwn_adam_rate(lr, step, b1, b2) read from DEVICE memory
 * (one float), so that the launch can be recorded in a hipGraph and replayed while the rate changes. */
double fwn_adam_rate(float lr, int64_t step, float beta1, float beta2);
int fwn_clip_adam_dev(float* w, const float* g, float* m, float* v, int64_t n, const float* gnorm, float gscale,
                      float clip, const float* lr_t, float beta1, float beta2, float eps, void* stream);
/* Gradient accumulation (additive; FWN_VERSION unchanged): one optimiser update over K micro-batches sums their gradients in a
 * second flat buffer and passes K where the loss scale goes (gscale = 1 / (world * K)).
 * dst[i] = a ? a[i] + b[i] : b[i], one IEEE fp32 add per element, i in [0, n).  dst may be a or b (in place); any other
 * overlap of dst with a source is refused.  Pointers need 4-byte alignment only: with one shared misalignment mod 16 (a range
 * of the flat layout in all three buffers) the kernel runs a scalar head of up to 3 elements, a 16-byte body and a scalar
 * tail, otherwise it moves dwords.  FWN_ERR_ARG before any launch: NULL dst or b, n <= 0, a pointer not 4-byte aligned,
 * partial overlap. */
int fwn_grad_accumulate(float* dst, const float* a, const float* b, int64_t n, void* stream);

/* ---- training-side primitives (work in progress: the backward pass) ----
 * Generic multi-segment GEMM on the LDS-DMA ring core:
 *   Y[M][N] = oscale * relu?( mask?( sum_s shift_s(X_s)[M][k_s] . W[N][koff_s ..]^T + bias + rscale * R ) )
 * X_s: bf16 [rows_s][ld_s], row r of the product reads row r + shift_s (a tap); with Ti > 0 rows are
 * clips of Ti rows and taps that leave their clip read zero, with Ti == 0 only the matrix bounds apply.
 * W: bf16 [N][ldw], segment s in columns [koff_s, koff_s + k_s) (k_s a multiple of 8; padding finite).
 * mask: keep where mask[row][col] > 0 (the ReLU derivative from a stored activation).
 * Output bf16 [M][ldy], or fp32 (out_f32; accumulate: +=).  nsplit > 1 (fp32 only, no bias / R / mask):
 * the K chunks are split over nsplit partial outputs Y + z*split_stride, to be summed by
 * fwn_reduce_splits (fixed order: deterministic).
 * gate_aux != NULL (bf16 output only): the 256 output columns from gate_col0 (a multiple of 256) are a gradient d with
 * respect to a gated layer's output o = tanh(f) sigmoid(g); they are not stored in Y but, rounded to bf16 like Y, go
 * through the gate's derivative with gate_aux = [tanh f | sigmoid g] (bf16 [M][512], kept by fwn_gate_train):
 * gate_out[M][512] (bf16) = [d sg (1 - tf^2) | d tf sg (1 - sg)] - what fwn_gate_bwd computes from a stored d.
 * row_len != NULL (ragged batches; additive, FWN_VERSION unchanged: a host that zero-fills the descriptor keeps today's bits):
 * DEVICE int32 [M / Ti] lengths in samples, one per clip of Ti rows, a row holding len_spr samples.  Output rows
 * [row_len[b] / len_spr, Ti) of clip b are stored as exact 0 whatever the product gives there (in Y, or through the gate
 * derivative in gate_out) - the data-gradient form of a forward pass that overwrote those rows with a constant: a forward fill
 * of rows becomes a backward drop of the gradient at those rows.  Needs Ti > 0, M a multiple of Ti, len_spr > 0, nsplit == 1;
 * refused together with accumulate (what is already in Y at those rows is not a product of this call). */
#define FWN_GEMM_MAXSEG 8
typedef struct fwn_gemm_seg { const void* x; int32_t rows, ld, k, shift, koff, pad_; } fwn_gemm_seg;
typedef struct fwn_gemm_desc {
    fwn_gemm_seg seg[FWN_GEMM_MAXSEG];
    int32_t nseg, M, N, Ti;
    const void* W;      int32_t ldw, pad0_;
    const float* bias;
    const void* R;      int32_t ldr;    float rscale;
    const void* mask;   int32_t ldmask; int32_t relu;
    void* Y;            int32_t ldy;    int32_t out_f32;
    int32_t accumulate, nsplit;
    int64_t split_stride;
    float oscale;       int32_t gate_col0;
    const void* gate_aux; void* gate_out;
    const int32_t* row_len; int32_t len_spr, pad1_;
} fwn_gemm_desc;
int fwn_gemm(const fwn_gemm_desc* g, void* stream);
/* Host only: the tile fwn_gemm would launch for this descriptor as BM * 1000 + BN (256128, 128128, 64128, or 32064: the 32 x 64
 * tile with a 4-way split-K inside the workgroup), -1 with fwn_last_error set for a descriptor fwn_gemm refuses.  The sibling of
 * fwn_tn_gemm_tile; additive, FWN_VERSION unchanged. */
int fwn_gemm_tile(const fwn_gemm_desc* g);
/* For tap z < ntap (shift = shift0 + z*dshift): dst[z*C + c][m] = src[m + shift][c] (zero where the tap
 * leaves its clip / the matrix; columns m >= M zero), dst bf16 [ntap*C (+1)][ld_dst]; ones_row: the row after
 * the last tap = 1 for m < M (bias gradients ride the weight-gradient GEMM). */
int fwn_transpose_shift(const void* src, int M, int C, int ld_src, int shift0, int dshift, int ntap, int Ti, void* dst,
                        int ld_dst, int ones_row, void* stream);
int fwn_reduce_splits(const float* partial, int nsplit, int64_t stride, int64_t n, float scale, float* out,
                      void* stream);

/* Training forward of a gated layer: as fwn_gate (conditioning fused from ca, or hoisted: P = c_a Wc of this layer
 * from fwn_cond; exactly one of the two), also storing aux [M][512] bf16 = (tanh f | sigmoid g) in natural channel
 * order for fwn_gate_bwd. */
int fwn_gate_train(const fwn_flow_desc* d, int layer, const void* h, const void* ca, const float* P, void* o, void* aux,
                   int M, int Ti, void* stream);
/* Element-wise pieces.  Planes are fp32 [M][Ch]; `an` points at one plane's table [4][Ch] = (shift,
 * scale, 1/scale, 3 logs) (fwn_flow_desc.an + role*4*Ch); Z is the ZeroConv output before its exp(3 scale)
 * factor ez [2Ch] (modules.py:51-56), fp32 [M][2Ch]: (log_s | t) = Z * ez.
 * fwn_actnorm_apply: x <- (x + shift) scale.                                  (model.py:86-94)
 * fwn_coupling_fwd : y_b <- (y_b - t) exp(-log_s); partial[nblocks] <- sums of -log_s   (:124-141)
 * fwn_coupling_bwd : g = dL/d out_b <- dL/d y_b; out_b <- y_b; dZ (bf16, ld ldz) <- (dL/dlog_s | dL/dt)
 *                    with the log-det term cls = 1/(2 M Ch) added; dzz <- dZ * Z (ZeroConv scale gradient)
 * fwn_gate_bwd     : dpre [M][512] <- (do sg (1 - tf^2) | do tf sg (1 - sg)), do bf16 [M][256] with row stride
 *                    ld_do (a column block of a wider matrix is fine)                  (modules.py:124)
 * fwn_colsum_prod  : out[c] <- scale * sum_m A[m][c] * (B ? B[m][c] : 1), fp32 [M][C], fixed order;
 *                    partial: scratch of fwn_colsum_partials(M, C) floats
 * fwn_actnorm_bwd  : dy <- dy * scale; y <- y / scale - shift (the plane before ActNorm)
 * fwn_wn_backward_group (below, with the grouped weight-gradient GEMM): weight-norm backward straight from
 *                    the split-K partials of the weight-gradient GEMM: dW[k][n] = scale * sum_s part[s][row_src ?
 *                    row_src[k] : k][col0 + n] (part rows have ldp columns), db[n] = the same sum over row
 *                    bias_row (< 0 / NULL: none); V fp32 [K][N], g [N] -> dV, dg; g == NULL: dV = dW (no
 *                    weight norm)   (convolutional.py:73-80) */
int fwn_actnorm_apply(float* x, const float* an, int64_t n, int Ch, void* stream);
/* Both planes of a flow in one launch: an2 = the flow's table [2][4][Ch] (fwn_flow_desc.an), n elements per plane. */
int fwn_actnorm_apply2(float* xa, float* xb, const float* an2, int64_t n, int Ch, void* stream);
int fwn_coupling_fwd(float* yb, const float* Z, const float* ez, int64_t M, int Ch, float* partial, int nblocks,
                     void* stream);
int fwn_coupling_bwd(float* g, float* out_b, const float* Z, const float* ez, int64_t M, int Ch, float cls, void* dZ,
                     int ldz, float* dzz, void* stream);
/* fwn_coupling_bwd of a ragged batch: M = B rows, clip b holds len[b] samples (DEVICE int32 [B], clamped to [0, rows
 * samples_per_row] on the device) = its first len[b] / samples_per_row rows.  Inside a clip the log-det term is per clip,
 * cls = (float)(1 / ((double)B len[b])) - with len[b] = rows samples_per_row = 2 rows Ch the bits of fwn_coupling_bwd's 1 / (2 M Ch).
 * Rows past a clip's end: g, out_b, both halves of dZ and of dzz are written as exact 0 (the forward pass zeroed out_b there,
 * so whatever gradient arrives at those rows is dropped).  ya / ya_bf (both or neither): also ya_bf [M][ldya] (bf16, ldya >= Ch,
 * zero padded) = the other plane, 0 in the rows past a clip's end, and the zero padding of dZ's columns [2 Ch, ldz). */
int fwn_coupling_bwd_ragged(float* g, float* out_b, const float* Z, const float* ez, int64_t B, int64_t rows, int Ch,
                            const int32_t* len, int32_t samples_per_row, void* dZ, int ldz, float* dzz, const float* ya,
                            void* ya_bf, int ldya, void* stream);
int fwn_gate_bwd(const void* d_o, int ld_do, const void* aux, int64_t M, void* dpre, void* stream);
int fwn_colsum_partials(int64_t M, int C);
int fwn_colsum_prod(const float* A, const float* B, int64_t M, int C, float scale, float* partial, float* out,
                    void* stream);
int fwn_actnorm_bwd(float* dy, float* y, const float* an, int64_t n, int Ch, void* stream);
/* The parameter-sized gradients around a flow's ActNorm, fused (two launches): for both planes (g, y = ActNorm
 * output; an [2][4][Ch]) s1 = sum_m g, s2 = sum_m g y, then fwn_actnorm_bwd in place; z = column sums of dzz
 * [M][2 Ch].  Outputs in the parameters' order through the index tables br [Ch] / zc [2 Ch] (int64, device):
 * db[role Ch + br[c]] = s1 scale, dlogs[role Ch + br[c]] = 3 s2 - 3/(2 Ch), dzscale[zc[j]] = 3 z[j].
 * partial: fwn_flow_small_grads_partials(M, Ch) doubles.  Ch: power of two <= 128. */
int64_t fwn_flow_small_grads_partials(int64_t M, int Ch);
int fwn_flow_small_grads(float* ga, float* ya, float* gb, float* yb, const float* dzz, const float* an, int64_t M, int Ch,
                         const int64_t* br, const int64_t* zc, double* partial, float* db, float* dlogs, float* dzscale,
                         void* stream);
/* fwn_flow_small_grads of a ragged batch (M = B rows; len, samples_per_row as in fwn_coupling_bwd_ragged): the rows past a
 * clip's end are left out of the five sums and written back as exact 0 in all four planes (the flow before this one saw 0
 * there in the forward pass, not the -shift that ActNorm's inverse gives).  The other rows are summed in fwn_flow_small_grads'
 * order: with every length = rows samples_per_row the same bits. */
int fwn_flow_small_grads_ragged(float* ga, float* ya, float* gb, float* yb, const float* dzz, const float* an, int64_t B,
                                int64_t rows, int Ch, const int32_t* len, int32_t samples_per_row, const int64_t* br,
                                const int64_t* zc, double* partial, float* db, float* dlogs, float* dzscale, void* stream);

/* Backward of one up-sampling stage (fwn_upsample_stage with fp32 output): y, dy [B][H*s][W], x [B][H][W].
 * dy <- dy * LeakyReLU'(y) in place; dx (may be NULL) <- gradient wrt x; dwk_bias [6s + 1] <- gradients of
 * the (weight-normed) kernel [2s][3] followed by the bias, two fixed-order passes through `partial`
 * (fwn_upsample_bwd_partials(B, H, s) floats).                                      (model.py:301-311) */
int fwn_upsample_bwd_partials(int B, int H, int s);
int fwn_upsample_bwd(float* dy, const float* y, const float* x, int B, int H, int W, int s, const float* wk,
                     float* dx, float* dwk_bias, float* partial, void* stream);

/* Weight-gradient GEMM without transposed copies: part[z][tap*Kx + i][j] = sum over the z-th share of the
 * rows m of X[m + shift0 + tap*dshift][i] * dY[m][j]  (bf16 X [M][ldx], dY [M][ldy]; taps that leave their clip of
 * Ti rows contribute zero; Ti == 0: matrix bounds only), fp32 partials [nsplit][ntap*Kx (+1)][N] for fwn_wn_backward /
 * fwn_reduce_splits; bias_row != 0 appends the column sums of dY (the bias gradient) as row ntap*Kx.  The operands are read transposed out of LDS (ds_read_b64_tr_b16).
 * fwn_colsum_bf16: out[c] = scale * sum_m dY[m][c] (bias gradients), scratch fwn_colsum_partials(M, C) floats. */
int fwn_tn_gemm(const void* x, int ldx, int Kx, int ntap, int shift0, int dshift, const void* dy, int ldy, int N, int M,
                int Ti, int nsplit, float* part, int64_t split_stride, int bias_row, void* stream);

/* Grouped forms: the weight gradients of one flow (same M, Ti) in ONE launch each - the job table travels in the
 * kernel arguments (at most FWN_MAX_GROUP jobs), every job needs only a few splits for the group to fill the chip. */
#define FWN_MAX_GROUP 16
typedef struct fwn_tn_job {
    const void* x; const void* dy; float* part; int64_t split_stride;
    int32_t ldx, Kx, ntap, shift0, dshift, ldy, N, nsplit, bias_row, reserved;
} fwn_tn_job;
int fwn_tn_gemm_group(const fwn_tn_job* jobs, int njobs, int M, int Ti, void* stream);
/* Edge of the square output tile the group launch uses at this M (128 or 256): what a caller sizes nsplit with. */
int fwn_tn_gemm_tile(int M);
typedef struct fwn_wn_job {
    const float* part; const int32_t* row_src; const float* V; const float* g; float* dV; float* dg; float* db;
    int64_t split_stride;
    int32_t nsplit, ldp, col0, bias_row, K, N; float scale; int32_t reserved;
    const int32_t* col_src;      /* NULL, or output column n reads partial column col0 + col_src[n] (a column permutation) */
} fwn_wn_job;
/* fwn_wn_backward for every job of the group (two launches); scratch: fwn_wn_group_scratch(jobs, njobs) doubles. */
int64_t fwn_wn_group_scratch(const fwn_wn_job* jobs, int njobs);
int fwn_wn_backward_group(const fwn_wn_job* jobs, int njobs, double* scratch, void* stream);
int fwn_colsum_bf16(const void* dy, int64_t M, int C, int ld, float scale, float* partial, float* out, void* stream);

/* ---- whole model (replaces FloWaveNet.forward / .reverse, model.py:317-396) ---- */
typedef struct fwn_model_desc {
    int32_t n_block, n_flow, n_layer, num_mels;
    int32_t n_up;
    int32_t up_scale[FWN_MAX_UPSAMPLE];
    const float* up_w[FWN_MAX_UPSAMPLE];      /* device [2s][3] weight-normed kernels */
    float up_bias[FWN_MAX_UPSAMPLE];
    const fwn_flow_desc* flows;               /* HOST array [n_block*n_flow] */
    int32_t cond_mode;                        /* 0 auto, 1 always fused in gate, 2 always hoisted */
    int32_t gate_fp8;                         /* != 0: fp8 dilated taps where supported (needs flows[].Wd8) */
    int32_t chain_mode;                       /* 0: chain the flows of a block (out_b to a third plane buffer, the next flow's
                                               * front conv in the previous flow's tail: csrc/tail_chain.h); 1: every flow on its own */
    int32_t persist_mode;                     /* flows of small-M blocks (hoisted conditioning) as ONE launch each (csrc/flow_persist.h;
                                               * same results bit for bit as a launch per stage): 0 = where that measured faster
                                               * (<= 512 rows: DESIGN.md section 3.7), 1 = never, 2 = wherever the form exists
                                               * (<= 4096 rows, n_layer <= 2) */
    /* Diagnostic (bench.py's per-block table), normally NULL: HOST array of n_block + 1 hipEvent_t handles.  The whole-model
     * calls record [k] on `stream` in front of the first launch of the k-th block they run (forward: block k, reverse: block
     * n_block - 1 - k) and [n_block] behind the last launch of the last one. */
    void* const* block_events;
    /* Per block: NULL, or the fragment streams (fwn_pack_cond_stream) of the block's n_flow * n_layer conditioning matrices in
     * (flow, layer) order: the hoisted projection of the block then runs the register-streamed kernel from fwn_cond_stream_rows()
     * rows on (0.3.21; a 0.3.20 host that zero-fills the descriptor keeps the ring tiles). */
    const void* cond_stream[16];
} fwn_model_desc;

size_t fwn_workspace_bytes(const fwn_model_desc* m, int64_t B, int64_t T);
/* x [B][T] fp32, mel [B][T/hop][num_mels] fp32 -> out2 = (log_p, logdet) fp32 on device.
 * z_planes (optional) receives the final flow state planes[2][B][T/2].  init != 0 performs the
 * ActNorm data-dependent init flow by flow (train.py:221,229 with init=True). */
int fwn_model_forward(const fwn_model_desc* m, int64_t B, int64_t T, const float* x, const float* mel,
                      void* workspace, size_t workspace_bytes, float* out2, float* z_planes, int init,
                      void* stream);
/* fwn_model_forward with init != 0 for one rank of a data-parallel job: before each flow's ActNorm tables are
 * derived, `reduce(user, buf, n, stream)` is called on the host with the DEVICE buffer of n doubles holding this
 * rank's moments (inside `workspace`); it must enqueue, in `stream` order, an in-place sum over all ranks (RCCL
 * all-reduce) and return 0.  reduce == NULL: single rank (moments of the local batch). */
typedef int (*fwn_reduce_fn)(void* user, double* buf, int n, void* stream);
int fwn_model_forward_init(const fwn_model_desc* m, int64_t B, int64_t T, const float* x, const float* mel,
                           void* workspace, size_t workspace_bytes, float* out2, float* z_planes,
                           fwn_reduce_fn reduce, void* user, void* stream);
/* z [B][T] fp32, mel -> x_out [B][T] fp32. */
int fwn_model_reverse(const fwn_model_desc* m, int64_t B, int64_t T, const float* z, const float* mel,
                      void* workspace, size_t workspace_bytes, float* x_out, void* stream);
/* The same question for a whole-model call (0.3.20): the per-flow sync blocks of fwn_model_forward / fwn_model_reverse live inside
 * their workspace.  After a pass with the same (m, B, T, workspace): 0 = no one-launch flow gave up, > 0 = the give-up code of the
 * first that did (log_p / logdet / the waveform are NaN then: retry, e.g. with fwn_model_desc.persist_mode = 1).  Synchronises. */
int fwn_model_persist_status(const fwn_model_desc* m, int64_t B, int64_t T, const void* workspace, void* stream);

/* ---- ragged batches: clips of different lengths in one inverse pass ----
 * Zero-fill of the rows past each clip's own length: rows [len[b] / samples_per_row, rows) of clip b in a
 * [B][rows][row_bytes] buffer (base 4-byte aligned, row_bytes a multiple of 4).  len: DEVICE array of B lengths in samples,
 * read by the kernel (the call stays asynchronous and graph-capturable) and clamped there to [0, rows * samples_per_row]: no
 * value of it writes outside the buffer.  The stores are proportional to the padding, 16 bytes each where aligned. */
int fwn_mask_rows(void* base, int64_t B, int64_t rows, int64_t row_bytes, const int32_t* len, int32_t samples_per_row,
                  void* stream);
/* Workspace of fwn_model_reverse_ragged: that of fwn_workspace_bytes plus the masked copy of the mel. */
size_t fwn_ragged_workspace_bytes(const fwn_model_desc* m, int64_t B, int64_t T);
/* fwn_model_reverse for B clips of len_dev[b] <= T samples each (DEVICE int32 [B], every length a multiple of hop and of
 * 2^n_block, validated by the caller): clip b is z[b][0 .. len) with mel[b][0 .. len / hop).  x_out[b][0 .. len) is what
 * the clip gives alone, to rounding; x_out[b][len .. T) is 0; nothing past a clip's length in z or mel reaches an output bit
 * (any finite values) and neither input is written.  Every stage reads a clip's neighbours in time only through rows that
 * are exact zeros past its end (the convolutions' own zero padding at T): the pass zero-fills those rows of the mel and of
 * each inner up-sampling stage, of the flow state (at the split and after every flow) and of h (after the front conv and
 * every res conv).  It runs every flow as a launch per stage - no one-launch flows, no chaining, whatever persist_mode and
 * chain_mode say.  A gate_fp8 descriptor is refused (FWN_ERR_ARG). */
int fwn_model_reverse_ragged(const fwn_model_desc* m, int64_t B, int64_t T, const float* z, const float* mel,
                             const int32_t* len_dev, void* workspace, size_t workspace_bytes, float* x_out, void* stream);

/* ---- ragged batches, forward direction: per-clip log_p and logdet (additive; FWN_VERSION unchanged) ----
 * fwn_model_forward for B clips of len_dev[b] <= T samples each (DEVICE int32 [B], validated by the caller as above).
 * out2B [2][B] fp32: out2B[b] = log_p and out2B[B + b] = logdet of clip b - what fwn_model_forward gives for
 * x[b][0 .. len) with mel[b][0 .. len / hop) alone, to rounding: the prior mean over the clip's own len samples, and per flow
 * mean_C(3 logs) + mean over the clip's own rows of -log_s, halved.  z_planes (may be NULL) [2][B][T/2]: the latent planes,
 * exactly 0 past each clip's end (fwn_model_reverse_ragged inverts them).  Nothing past a clip's length in x or mel reaches
 * an output bit and neither input is written.  The pass is fwn_model_reverse_ragged's in the other direction - a launch per
 * stage, the same zero-fills - with two additions.  The front conv applies ActNorm on the fly, so the rows past a clip's end of
 * each flow's x_a plane are filled with -shift first (fwn_fill_neg_shift): ActNorm of them is an exact 0, the zero padding a
 * clip on its own gets behind ActNorm.  And every flow's tail keeps its ZeroConv output (as fwn_tail_train does), from which
 * fwn_ragged_logdet_rows sums -log_s per clip over the clip's own rows; the tail's own whole-batch partials are ignored.
 * All sums are fp64 in a fixed order (no atomics): two identical calls give identical bits.  No data-dependent init; a
 * gate_fp8 descriptor is refused (FWN_ERR_ARG).  Workspace: fwn_ragged_forward_workspace_bytes (0 for a bad descriptor). */
size_t fwn_ragged_forward_workspace_bytes(const fwn_model_desc* m, int64_t B, int64_t T);
int fwn_model_forward_ragged(const fwn_model_desc* m, int64_t B, int64_t T, const float* x, const float* mel,
                             const int32_t* len_dev, void* workspace, size_t workspace_bytes, float* out2B, float* z_planes,
                             void* stream);
/* -shift[c] into rows [len[b] / samples_per_row, rows) of clip b of a [B][rows][Ch] fp32 plane (Ch a power of two, shift
 * [Ch]: the first row of a flow's ActNorm table).  len as in fwn_mask_rows: read and clamped on the device, no value of it
 * writes outside the plane.  plane 4-byte aligned. */
int fwn_fill_neg_shift(float* plane, int64_t B, int64_t rows, int Ch, const float* shift, const int32_t* len,
                       int32_t samples_per_row, void* stream);
/* One flow's log-det terms per clip.  Z [B][rows][2 Ch] fp32 (fwn_tail_train's save_z: log_s channels, then t channels),
 * ez: the flow's ezero.  acc [B][nslot] fp64 with nslot = fwn_ragged_logdet_slots(B): acc[b][0 .. nslot - 1) are chunk sums
 * of -Z[row][c] * ez(c) over rows [0, len[b] / samples_per_row) and c < Ch - their sum in index order is the clip's sum; no
 * row past a clip's end is loaded - and acc[b][nslot - 1] = sum_c of both planes' 3 logs from the ActNorm table an (NULL:
 * left unwritten). */
int fwn_ragged_logdet_slots(int64_t B);
int fwn_ragged_logdet_rows(const float* Z, int64_t B, int64_t rows, int Ch, const float* ez, const float* an,
                           const int32_t* len, int32_t samples_per_row, double* acc, void* stream);

/* ---- ragged batches: the ActNorm data-dependent init (additive; FWN_VERSION unchanged) ----
 * fwn_actnorm_moments over the clips' own rows.  xa, xb [B][rows][Ch] fp32 (4-byte aligned, Ch a power of two); len: DEVICE
 * int32 [B], read and clamped on the device as in fwn_mask_rows - clip b counts rows [0, len[b] / samples_per_row) and no row
 * past that is loaded.  mom[4 Ch + 1] doubles in the layout fwn_actnorm_from_moments reads: per plane (sum | sum of squares)
 * per channel over the counted rows, then the NUMBER of counted rows, sum_b clamp(len[b], 0, rows samples_per_row) /
 * samples_per_row, as the last double - so an all-reduce of the buffer weights ranks with different amounts of data
 * correctly.  The rows of a channel are split over several workgroups whose fp64 partial sums (scratch, at least
 * fwn_actnorm_moments_ragged_scratch_bytes(B, rows, Ch) bytes, 8-byte aligned; 0 for a bad shape) a second launch adds in a
 * fixed order: no atomics, two identical calls give identical bits. */
int64_t fwn_actnorm_moments_ragged_scratch_bytes(int64_t B, int64_t rows, int Ch);
int fwn_actnorm_moments_ragged(const float* xa, const float* xb, int64_t B, int64_t rows, int Ch, const int32_t* len,
                               int32_t samples_per_row, double* mom, double* scratch, int64_t scratch_bytes, void* stream);
/* fwn_model_forward_init for B clips of len_dev[b] <= T samples each (DEVICE int32 [B], validated by the caller as for
 * fwn_model_reverse_ragged): flow by flow in forward order, b = -mean and logs = log(1 / (sqrt(mean((x + b)^2)) + 1e-7)) / 3 per
 * channel with the means over the union of the clips' own rows, then the flow as fwn_model_forward_ragged runs it.  Per flow:
 * fwn_actnorm_moments_ragged; `reduce` (may be NULL: single rank) over the 4 Ch + 1 doubles as in fwn_model_forward_init - the
 * row count is summed with the moments; fwn_actnorm_from_moments into the flow's table; fwn_fill_neg_shift with that table;
 * the stages.  out2B [2][B] and z_planes (may be NULL) as in fwn_model_forward_ragged; nothing past a clip's length in x or mel
 * reaches a table or an output bit.  Null lengths and a gate_fp8 descriptor are refused (FWN_ERR_ARG).  Workspace:
 * fwn_ragged_init_workspace_bytes (0 for a bad or gate_fp8 descriptor).  fwn_model_forward_ragged and fwn_model_forward[_init]
 * are unchanged.  Speed: not measured - the pass runs once per training run. */
size_t fwn_ragged_init_workspace_bytes(const fwn_model_desc* m, int64_t B, int64_t T);
int fwn_model_forward_init_ragged(const fwn_model_desc* m, int64_t B, int64_t T, const float* x, const float* mel,
                                  const int32_t* len_dev, void* workspace, size_t workspace_bytes, float* out2B, float* z_planes,
                                  fwn_reduce_fn reduce, void* user, void* stream);

/* ---- training: loss = -(log_p + logdet) (train.py:56-60) and its gradient with respect to every trainable tensor
 * (the one tf.gradients call of train.py:63-66) for one batch, in ONE call: training forward with what the backward
 * needs kept per flow, then the flows in reverse (coupling, ZeroConv / final / skip / res, the gated layers with their
 * dilated transposed convs, the conditioning gradient, the front conv, ActNorm), then the up-sampling convs.  The
 * descriptors hold device pointers to (a) the inference packing of the parameters (fwn_model_desc, conditioning fused:
 * cond_mode 1), (b) the natural-order / transposed bf16 copies the backward GEMMs read, (c) the fp32 masters in the
 * reference's layouts and (d) where each gradient goes (e.g. views of one flat buffer that an RCCL all-reduce sums).
 * Everything else lives in `workspace`.  on_block_done(user, i) is called on the host once every launch that writes
 * block i's gradients has been enqueued (blocks finish last to first; -1 = the up-sampling convs): the hook a
 * data-parallel step uses to start that block's all-reduce under the rest of the backward pass, or to cut a graph.
 * The hook returns 0 to go on; any other value stops the sequencing at once (nothing further is enqueued) and
 * fwn_train_loss_and_grads returns FWN_ERR_CALLBACK - a host that cannot let an exception cross the C frame reports
 * it this way and re-raises after the call. */
typedef struct fwn_conv_grad {          /* one trainable convolution */
    const float* V; const float* g;     /* kernel [K][N] fp32 (reference layout, K = kernel_size * C_in), weight-norm g [N] or NULL */
    float* dV; float* dg; float* db;    /* gradients of kernel, g (NULL iff g NULL) and bias */
} fwn_conv_grad;
typedef struct fwn_flow_train_desc {
    const void* WfT;                            /* [Ch][768]   front conv, transposed: K = tap*256 + n          */
    const void* WdT[FWN_MAX_LAYERS];            /* [256][1536] dilated filter|gate, K = tap*512 + (f|g)*256 + n */
    const void* WcT[FWN_MAX_LAYERS];            /* [cin][512]  conditioning filter|gate, row stride wct_ld      */
    const void* WresT[FWN_MAX_LAYERS];          /* [256][256]  layers 0..L-2                                    */
    /* Wskip / Wfin / Wz / bskip / bfin / bz: unused since the forward half runs the inference tail (fwn_tail_train) - may
     * be NULL; the backward reads the transposed copies and ez */
    const void* Wskip;  const void* WskipT_all; /* (unused), [L*256][256]                                       */
    const void* Wfin;   const void* WfinT;      /* (unused), [256][256] transposed                              */
    const void* Wz;     const void* WzT;        /* (unused), [256][ldz] columns in plane order                  */
    const float* bskip; const float* bfin; const float* bz; const float* ez;    /* ez [2Ch] = exp(3 scale), plane order */
    int32_t ldz;                                /* max(8, 2Ch)                                                  */
    int32_t wct_ld;                             /* row stride of WcT in elements (0: 512).  L*512 with WcT[l] =
                                                   WcT[0] + l*512: the layers side by side in one [cin][L*512] matrix -
                                                   the conditioning gradient of a flow is then ONE GEMM over K = L*512 */
    fwn_conv_grad front, final_, zero;          /* Conv_front, Conv_final, ZeroConv1d (g = NULL)                */
    fwn_conv_grad filt[FWN_MAX_LAYERS], gate[FWN_MAX_LAYERS], res[FWN_MAX_LAYERS], skip[FWN_MAX_LAYERS],
        filt_c[FWN_MAX_LAYERS], gate_c[FWN_MAX_LAYERS];
    float* d_an_b; float* d_an_logs; float* d_zscale;    /* [2Ch] each, the parameters' order                  */
} fwn_flow_train_desc;
typedef struct fwn_train_desc {
    const fwn_model_desc* model;                /* inference packing of the same parameters                     */
    const fwn_flow_train_desc* flows;           /* HOST array [n_block * n_flow]                                */
    /* per block (device): logical row of a weight gradient -> row of the GEMM that computed it; channel maps   */
    const int32_t* cond_rows[16]; const int32_t* front_rows[16]; const int32_t* zinv32[16];
    const int64_t* br[16]; const int64_t* zcol[16];
    const float* up_bias_dev[FWN_MAX_UPSAMPLE]; /* the bias masters (device scalars)                            */
    fwn_conv_grad up[FWN_MAX_UPSAMPLE];         /* V [2s][3], scalar g; dV, dg, db (bias)                       */
    int32_t zero_dead_res;                      /* != 0: also zero the gradients of the dead last-layer res_conv */
    /* Optional second hipStream_t (NULL: one stream).  The weight gradients of block i (grouped TN GEMMs + weight-norm
     * backward) and its conditioning-gradient GEMMs then run on it under the data-gradient chain of block i - 1 and are
     * joined into `stream` before on_block_done(i); the workspace grows by per-flow copies of the temporaries they
     * read.  Same results.  On an error return every path first joins the side stream into `stream`: nothing of the
     * call is left running on it. */
    void* side_stream;
} fwn_train_desc;
typedef int (*fwn_block_done_fn)(void* user, int block);
size_t fwn_train_workspace_bytes(const fwn_train_desc* t, int64_t B, int64_t T);
/* x [B][T] fp32, mel [B][T/hop][num_mels] fp32 -> out3 = (loss, log_p, logdet) fp32 on device + every gradient. */
int fwn_train_loss_and_grads(const fwn_train_desc* t, int64_t B, int64_t T, const float* x, const float* mel,
                             void* workspace, size_t workspace_bytes, float* out3, fwn_block_done_fn on_block_done,
                             void* user, void* stream);
/* ---- ragged training step (additive; FWN_VERSION unchanged): clips of len_dev[b] <= T samples each (DEVICE int32 [B], every
 * length a multiple of hop and of 2^n_block, validated by the caller; only kernels read it, so the call stays asynchronous and
 * graph-capturable).  loss = -(1/B) sum_b (log_p[b] + logdet[b]) with the per-clip scalars of fwn_model_forward_ragged, and
 * every gradient is the mean over b of clip b's own gradient (every length = T: the gradients of fwn_train_loss_and_grads bit
 * for bit).  out3 = (loss, mean log_p, mean logdet); out2B (may be NULL) [2][B] as in fwn_model_forward_ragged.  Nothing past a
 * clip's end in x or mel reaches an output bit and neither is written.
 * The same sequencer as fwn_train_loss_and_grads.  Forward half: fwn_model_forward_ragged's fills - a masked copy of the mel and
 * masked inner up-sampling stages (the buffers the up-sampling backward reads), -shift in x_a's padding in front of each front
 * conv, h zeroed behind the front conv and every res conv before it is kept, the planes zeroed after every flow; the per-clip
 * scalars come from fwn_ragged_logdet_rows over the Z each tail keeps for the backward.  Backward half: the adjoint of those
 * fills - a forward fill of rows becomes a backward drop of the gradient at those rows: d loss / d z = z / (B len[b]) inside a
 * clip and 0 past it; fwn_coupling_bwd_ragged; the dilated data-gradient GEMMs store dh with fwn_gemm_desc.row_len;
 * fwn_flow_small_grads_ragged; fwn_mask_rows on the dx of each inner up-sampling stage.  No launch is added to a flow's chain.
 * A gate_fp8 descriptor is refused (FWN_ERR_ARG).  Workspace: fwn_train_ragged_workspace_bytes (0 for a bad descriptor).
 * Speed (tools/bench_train.py --ragged, 8 x 6400 samples, one MI355X: profiles/ragged_training.json): 14.6 ms against the plain
 * step's 12.8; not measured on more than one GPU. */
size_t fwn_train_ragged_workspace_bytes(const fwn_train_desc* t, int64_t B, int64_t T);
int fwn_train_loss_and_grads_ragged(const fwn_train_desc* t, int64_t B, int64_t T, const float* x, const float* mel,
                                    const int32_t* len_dev, void* workspace, size_t workspace_bytes, float* out3, float* out2B,
                                    fwn_block_done_fn on_block_done, void* user, void* stream);

/* ---- device-side synthesis (additive; FWN_VERSION unchanged): the latent z drawn on the device, 16-bit PCM written there, and
 * both around the inverse pass in one call - only the mel has to go up and only int16 has to come down.
 *
 * fwn_latent_normal: z [B][T] fp32 = temp * N(0,1) from Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants
 * 0x9E3779B9 / 0xBB67AE85, ten rounds).  Key = (seed & 0xffffffff, seed >> 32); counter = (q, 0, clip_id[b], 0) with q = i / 4
 * for sample i of clip b; clip_id_dev is a DEVICE uint32 [B], NULL: clip_id[b] = b.  The four output words r0..r3 give samples
 * 4q .. 4q+3: for the pairs (r0, r1) and (r2, r3), u1 = ((r >> 8) + 1) 2^-24 in (0, 1], u2 = (r' >> 8) 2^-24, rad =
 * sqrt(-2 ln u1), and the two samples are rad cos(2 pi u2) and rad sin(2 pi u2), times temp.  Sample i of a clip depends on
 * (seed, clip_id, i, temp) only - not on B, the clip's row, T or the pointer's alignment: a clip draws the same z whichever
 * batch it lands in.  The stream is this library's own (neither TensorFlow's nor torch's).  Any T in [1, 2^34] and any 4-byte
 * aligned z; B < 65536.  len_dev (may be NULL): DEVICE int32 [B], read and clamped to [0, T] on the device as in fwn_mask_rows; samples
 * at i >= len[b] are +0.0f, the ones before it have the bits they have without len.  fp32 evaluation with accurate log / sqrt /
 * sincos: within 1e-5 temp of the fp64 value of the formula (tests/philox_ref.py).
 *
 * fwn_pcm16: pcm [B][T] int16 = rint((double)clamp(x, -1, 1) * 32767.0), halves to even, NaN -> 0 - the arithmetic of the
 * synthesize CLI's float64 wav writer bit for bit.  x 4-byte, pcm 2-byte aligned, any T >= 1, B < 65536; len_dev as above:
 * samples at i >= len[b] are 0.
 *
 * fwn_model_synthesize: fwn_latent_normal -> fwn_model_reverse (len_dev NULL) or fwn_model_reverse_ragged -> fwn_pcm16, enqueued
 * on one stream.  mel [B][T/hop][num_mels] fp32; pcm_out [B][T] int16; wav_out / z_out (each may be NULL) [B][T] fp32 receive
 * the waveform and the latent; all three 16-byte aligned.  Without them z and the waveform live in the workspace, behind the
 * inverse pass's own: fwn_synthesize_workspace_bytes(m, B, T, ragged != 0 for a call with len_dev), 0 for a descriptor or shape
 * the call would refuse.  Refusals (FWN_ERR_ARG, before anything is launched): those of the two inverse entries - a gate_fp8
 * descriptor with len_dev, odd n_block * n_flow, B >= 32768 - and null or misaligned pointers.  Lengths are validated by the
 * caller as for fwn_model_reverse_ragged.  CLI-level speed: tools/bench_synth.py. */
int fwn_latent_normal(float* z, int64_t B, int64_t T, uint64_t seed, const uint32_t* clip_id_dev, float temp,
                      const int32_t* len_dev, void* stream);
int fwn_pcm16(const float* x, int16_t* pcm, int64_t B, int64_t T, const int32_t* len_dev, void* stream);
size_t fwn_synthesize_workspace_bytes(const fwn_model_desc* m, int64_t B, int64_t T, int ragged);
int fwn_model_synthesize(const fwn_model_desc* m, int64_t B, int64_t T, const float* mel, uint64_t seed,
                         const uint32_t* clip_id_dev, float temp, const int32_t* len_dev, void* workspace, size_t workspace_bytes,
                         int16_t* pcm_out, float* wav_out, float* z_out, void* stream);

/* ---- windowed synthesis (additive; FWN_VERSION unchanged): a clip of any length, or one whose mel is still arriving, as
 * windows with real context on both sides, each a plain rectangular fwn_model_reverse; only the cores are kept.  The planning
 * (which windows, how much context: tf_flowavenet_amd/windowing.py) is the host's; this is the device code around the pass.
 * Every table below is a DEVICE array read by the kernels; nothing is allocated or synchronised, so a call is capturable.
 *
 * fwn_latent_normal_at: fwn_latent_normal with a per-row start.  Row r of z [n][L] holds samples start[r] .. start[r] + L of
 * clip clip_id[r]'s stream (clip_id_dev NULL: clip r), bit for bit the slice of what fwn_latent_normal writes for that clip:
 * sample i = start + j from counter (i / 4, 0, clip_id, 0), lane i % 4, the same fp32 evaluation.  start_dev: DEVICE int64 [n],
 * any value >= 0 (a negative one is read as 0), not only multiples of 4; start + L <= 2^34 is the caller's to keep.  len_dev
 * (may be NULL) as in fwn_latent_normal, relative to the row: samples at j >= len[r] are +0.0f.  n < 65536; z 4-byte aligned.
 *
 * fwn_window_gather: row r of dst [n][rows][row_floats] fp32 = the rows * row_floats floats of src from row src_row_dev[r]
 * (DEVICE int64 [n]; 64-bit addressing: src is a flat buffer of rows of row_floats floats - for the mel, row_floats = num_mels
 * and the offset is the clip's first frame plus lo / hop).  16-byte accesses for a row of dst whose source and destination are
 * both 16-byte aligned (and whose size is a multiple of 16 bytes), dwords otherwise.  One launch.  rows * row_floats < 2^31.
 *
 * fwn_window_scatter_pcm16: for row r of x [n][L] fp32, pcm[out_off[r] + i] = pcm16(x[r][core_off[r] + i]) for i < core_len[r]
 * - fwn_pcm16's arithmetic bit for bit - and, if wav != NULL, wav[out_off[r] + i] = x[r][core_off[r] + i].  pcm or wav may be
 * NULL, not both.  core_off_dev / core_len_dev: DEVICE int32 [n], clamped into the row on the device; out_off_dev: DEVICE int64
 * [n], element offsets into the flat int16 / fp32 buffers (the caller's to keep inside them).  Nothing outside the cores is
 * written.  One launch.
 *
 * fwn_model_synthesize_windows: one group of n windows of L samples on one stream - fwn_latent_normal_at (start_dev, clip_id_dev;
 * no len) -> fwn_window_gather (mel_flat, mel_row_dev, rows L / hop of num_mels floats) -> fwn_model_reverse(m, n, L) ->
 * fwn_window_scatter_pcm16 (pcm_flat; wav_flat may be NULL).  z, the waveform and the gathered mel live in the workspace behind
 * the inverse pass's own: fwn_synthesize_windows_workspace_bytes(m, n, L) - a function of (n, L) alone, never of a clip's
 * length; 0 for a descriptor or shape the call would refuse.  Refusals (FWN_ERR_ARG, before anything is launched): those of
 * fwn_model_synthesize without lengths (the inverse pass's own, odd n_block * n_flow, n >= 32768), a null mel_flat, workspace,
 * pcm_flat or table, a table off its element's alignment (8 bytes for the int64 ones, 4 for the others), a workspace off 256
 * bytes.  Speed: tools/bench_windowed.py. */
int fwn_latent_normal_at(float* z, int64_t n, int64_t L, uint64_t seed, const uint32_t* clip_id_dev, const int64_t* start_dev,
                         float temp, const int32_t* len_dev, void* stream);
int fwn_window_gather(const float* src, const int64_t* src_row_dev, float* dst, int64_t n, int64_t rows, int64_t row_floats,
                      void* stream);
int fwn_window_scatter_pcm16(const float* x, int64_t n, int64_t L, const int32_t* core_off_dev, const int32_t* core_len_dev,
                             const int64_t* out_off_dev, int16_t* pcm, float* wav, void* stream);
size_t fwn_synthesize_windows_workspace_bytes(const fwn_model_desc* m, int64_t n, int64_t L);
int fwn_model_synthesize_windows(const fwn_model_desc* m, int64_t n, int64_t L, const float* mel_flat, const int64_t* mel_row_dev,
                                 const uint32_t* clip_id_dev, const int64_t* start_dev, const int32_t* core_off_dev,
                                 const int32_t* core_len_dev, const int64_t* out_off_dev, uint64_t seed, float temp, void* workspace,
                                 size_t workspace_bytes, int16_t* pcm_flat, float* wav_flat, void* stream);

/* ---- windowed forward (additive; FWN_VERSION unchanged): log_p, logdet and the latent of a clip of any length, as the windows
 * of windowed synthesis (the forward pass has the inverse pass's receptive field: the same halo, the same plans), each a plain
 * rectangular forward pass in the form that keeps every tail's ZeroConv output - the ragged forward's, on full-length rows, so
 * without a fill or a mask launch.  A window's own log_p / logdet would include its halo; the sums below go over the cores only
 * and are added per clip.  For a clip of t samples cut into windows with cores [a, b):
 *     log_p  = 0.5 (-log 2 pi - sum_windows sum_core z^2 / t)
 *     logdet = sum_flows mean_C(3 logs) + sum_windows sum_flows sum_{core rows, c} (-log_s) / t
 * (a flow of block i has t / 2^(i+1) rows of 2^i log_s channels, so the reference's mean(-log_s) / 2 is sum(-log_s) / t at every
 * block; core edges are multiples of lcm(hop, 2^n_block), so a core is whole rows everywhere).  Every sum is fp64 in an order
 * the launches fix - no atomics - so two identical calls give identical bits.  Every table below is a DEVICE array read and
 * clamped by the kernels; nothing is allocated or synchronised, so a call is capturable.
 *
 * fwn_window_logdet_rows: fwn_ragged_logdet_rows with a per-window start.  For window r of Z [n][rows][2 Ch]: the fp64 chunk sums
 * of -Z[row][c] ez(c) over rows [core_off[r] / samples_per_row, + core_len[r] / samples_per_row) -> acc[r][0 .. nslot - 1), the
 * ActNorm term (an may be NULL) -> acc[r][nslot - 1], nslot = fwn_ragged_logdet_slots(n).  The start is clamped to [0, rows] and
 * the count to what is left, on the device; no row outside the range is loaded.  core_off_dev / core_len_dev: DEVICE int32 [n],
 * samples.  One kernel serves both entries: fwn_ragged_logdet_rows(len) is the start-0 case, the same sums in the same order as
 * fwn_window_logdet_rows(core_off = 0, core_len = len) leaves.
 *
 * fwn_window_sums: window r's partial sums -> part[slot[r]][0 .. 4) fp64 (a negative slot writes nothing): [0] the sum of z^2
 * over elements [core_off / 2, (core_off + core_len) / 2) of both final planes [2][n][L / 2] (one contiguous range per plane;
 * clamped into the window, nothing outside is loaded), [1] the sum over the nflows flows, in flow order, of their chunk sums in
 * acc [nflows][n][nslot], [2] the sum over the flows of acc[f][r][nslot - 1] / (2 << (f / n_flow)) - the ActNorm terms, the
 * same for every window -, [3] the core's length.  slot_dev: DEVICE int32 [n]; part is the caller's table, as large as its
 * largest slot says.
 *
 * fwn_window_scatter_latent: the cores of the final planes in TIME order - z_flat[out_off[r] + i] = sample core_off[r] + i of
 * window r for i < core_len[r], where sample s lives in plane (s & 1) ^ swapped at element s / 2 (swapped: n_block * n_flow is
 * odd).  This is the reference's final `out` un-squeezed n_block times, the latent fwn_model_reverse takes.  out_off_dev:
 * DEVICE int64 [n], element offsets (the caller's to keep inside z_flat); nothing outside the cores is written.
 *
 * fwn_forward_windows_finish: one launch after the last group.  Clip c's windows are slots [slot0[c], slot0[c] + nwin[c]) of
 * part, in window order; they are added in that order, whatever groups they ran in, and out2B [2][n_clips] fp32 = (log_p,
 * logdet) per clip as fwn_model_forward_ragged lays it out; t is the sum of the cores' lengths.
 *
 * fwn_model_forward_windows: one group of n windows of L samples on one stream - fwn_window_gather of the audio (x_flat, rows
 * of hop floats from row x_row[r]: 64-bit) and of the mel (mel_flat, rows of num_mels floats from mel_row[r]) -> the pass ->
 * fwn_window_sums into acc[slot[r]] -> fwn_window_scatter_latent (z_flat may be NULL: no latent; then z_out_off_dev may be too).
 * acc: the caller's fp64 table [.][4] for fwn_forward_windows_finish.  fwn_forward_windows_workspace_bytes(m, n, L) is a
 * function of (n, L) alone and 0 for what the call refuses.  Refusals (FWN_ERR_ARG, before anything is launched): those of
 * fwn_model_forward's shape checks, a null x_flat, mel_flat, acc, workspace or table, a table off its element's alignment (8
 * bytes for the int64 ones and acc, 4 for the others), a workspace off 256 bytes, n >= 32768, a gate_fp8 descriptor.  Speed:
 * tools/bench_windowed_forward.py. */
int fwn_window_logdet_rows(const float* Z, int64_t n, int64_t rows, int Ch, const float* ez, const float* an, const int32_t* core_off_dev,
                           const int32_t* core_len_dev, int32_t samples_per_row, double* acc, void* stream);
int fwn_window_sums(const float* planes, int64_t n, int64_t L, const int32_t* core_off_dev, const int32_t* core_len_dev, const double* acc,
                    int nflows, int n_flow, const int32_t* slot_dev, double* part, void* stream);
int fwn_window_scatter_latent(const float* planes, int64_t n, int64_t L, int swapped, const int32_t* core_off_dev,
                              const int32_t* core_len_dev, const int64_t* out_off_dev, float* z_flat, void* stream);
int fwn_forward_windows_finish(const double* part, const int32_t* clip_slot0_dev, const int32_t* clip_nwin_dev, int64_t n_clips,
                               float* out2B, void* stream);
size_t fwn_forward_windows_workspace_bytes(const fwn_model_desc* m, int64_t n, int64_t L);
int fwn_model_forward_windows(const fwn_model_desc* m, int64_t n, int64_t L, const float* x_flat, const int64_t* x_row_dev,
                              const float* mel_flat, const int64_t* mel_row_dev, const int32_t* core_off_dev, const int32_t* core_len_dev,
                              const int32_t* slot_dev, double* acc, const int64_t* z_out_off_dev, float* z_flat, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ---- device-resident corpus (additive; FWN_VERSION unchanged): a training batch drawn and gathered on the device.
 *
 * Layout.  audio: flat fp32, all utterances back to back; mel: flat fp32 [total_frames][num_mels]; frame_off: DEVICE int64
 * [n_utt + 1], non-decreasing.  Utterance u owns frames [frame_off[u], frame_off[u+1]) of mel and the samples from
 * hop * frame_off[u] of audio: the loader keeps min(mel frames, audio samples / hop) frames of each utterance, so one table
 * serves both arrays.  Every offset is int64 (a corpus of more than 2^31 samples is the ordinary case); one utterance holds
 * fewer than 2^31 frames.
 *
 * The draw (this library's own stream, like fwn_latent_normal's; restated in NumPy by tests/corpus_ref.py).  d = the uint64 at
 * *counter_dev.  Slot b < B takes r = Philox4x32-10(counter = (d & 0xffffffff, d >> 32, b, stream_id), key = (seed &
 * 0xffffffff, seed >> 32)) and of it
 *     u = (r0 * n_utt) >> 32                                   (64-bit product), n = frame_off[u+1] - frame_off[u];
 *     n > F :  start = (r1 * (n - F)) >> 32, frames = F        (a crop from [0, n - F), the range of dataset.py:73)
 *     n <= F:  start = 0, frames = (n / unit_frames) * unit_frames      (the whole utterance, floored to the unit)
 * The multiply-high map x -> (r * x) >> 32 of a uniform 32-bit r onto [0, x) is onto, monotone in r (r = 0 -> 0, r = 2^32 - 1
 * -> x - 1) and gives every value either floor(2^32 / x) or that plus one of the 2^32 words: a value's probability differs from
 * 1 / x by less than 2^-32, i.e. by a relative x / 2^32 at most (3e-6 for 13 100 utterances).  A slot's pick depends on (seed,
 * stream_id, d, b) only - not on B: the first slots of a larger batch are the smaller batch.
 *
 * Outputs, every element written by every call: x [B][F * hop] = the audio from sample hop * (frame_off[u] + start), c [B][F]
 * [num_mels] = the mel rows from frame_off[u] + start, both +0.0f past the clip's frames; len [B] int32 = frames * hop;
 * picks (may be NULL) [B][2] int32 = (u, start).  After the gather a one-lane kernel stores d + 1 to *counter_dev: the counter
 * moves on the device, in stream order, without atomics, and no lane of the draw can see the new value.  Nothing is allocated or
 * synchronised; two kernel launches on `stream`, capturable into a hipGraph whose every replay draws the next batch.
 * 16-byte loads and stores for a row whose source, destination and lengths are 16-byte multiples (hop or num_mels a
 * multiple of 4 with aligned bases), dwords otherwise.  Refusals (FWN_ERR_ARG, before any launch): a null audio, mel,
 * frame_off, counter_dev, x, c or len; B, F, n_utt, hop, num_mels or unit_frames < 1; B >= 65536; n_utt >= 2^31; F * hop or
 * F * num_mels >= 2^31; pointers off their element's alignment (4 bytes; 8 for frame_off and counter_dev). */
int fwn_corpus_draw(const float* audio, const float* mel, const int64_t* frame_off, int64_t n_utt, int hop, int num_mels,
                    int unit_frames, int64_t B, int64_t F, uint64_t seed, uint32_t stream_id, uint64_t* counter_dev, float* x,
                    float* c, int32_t* len, int32_t* picks, void* stream);

/* ---- sample-rate conversion (additive; FWN_VERSION unchanged): one band-limited rational resampler, so that wavs of any rate go
 * in (preprocessing.load_wav) and any rate comes out (synthesize --out_rate).  DESIGN.md "Sample-rate conversion" has the
 * definition; tests/resample_ref.py restates it in fp64.
 *
 * For in_rate -> out_rate: up = out_rate / gcd, down = in_rate / gcd, q = max(up, down), Hh = zeros * q.  A clip of N samples
 * has n_out(N) = ceil(N up / down) outputs
 *     y[m] = sum_n x[n] h[m down - n up],  |m down - n up| <= Hh,  x = 0 outside [0, N)
 *     h[j] = (up rolloff / q) sinc(rolloff j / q) I0(beta sqrt(1 - (j / Hh)^2)) / I0(beta),  sinc(t) = sin(pi t) / (pi t)
 * evaluated from the phase table T [up][K], K = 2 Hh div up + 1, T[r][k] = h[r + k up - Hh] (0 past the support): with n0 =
 * (m down + Hh) div up and r = (m down + Hh) mod up, y[m] = sum_k x[n0 - k] T[r][k].
 *
 * fwn_resample_taps: K, or FWN_ERR_ARG.  fwn_resample_design: T into table_host [up][K] - HOST memory, host code, no device
 * call: fp64 throughout (I0 by its power series), each entry rounded to fp32 once.  Both refuse (FWN_ERR_ARG, with a message) up
 * or down outside 1..2^20, gcd(up, down) != 1 and zeros outside 1..64; the design also rolloff outside (0, 1], beta < 0 (or
 * above 100, or NaN) and a null table.
 *
 * fwn_resample: one launch for B clips.  x: row b at x + b * x_stride elements, float32 (x_pcm16 = 0) or int16 PCM read as
 * v / 32768, exact (x_pcm16 = 1); element j of a row is CLIP sample in_start + j, j < n_in - the provided span.  Clip b has
 * N_b = len_dev[b] samples (DEVICE int64 [B], read on the device and clamped to [0, len_host]) or len_host when len_dev is
 * NULL.  y: row b at y + b * y_stride floats; y[b][i] = output m0 + i for i < n_out, and exact +0 where m0 + i >= n_out(N_b).
 * Nothing else is written.  No sample at or past N_b, and none outside the provided span, is loaded (a NaN there is harmless).
 * An output's bits depend only on the clip's samples in its support, on N_b and on m: not on B, the row, in_start, m0 or the
 * workgroup tile - each output is four fmaf chains over k mod 4 in ascending k, added (a0 + a1) + (a2 + a3) - so a clip cut
 * into chunks, or batched with others, gets the bits it gets alone.  All arithmetic on m down and N up is 64-bit: N up to
 * 2^40.  Refusals (FWN_ERR_ARG, before any launch): those of fwn_resample_taps; a null or misaligned x, y, table_dev (or
 * misaligned len_dev); x_pcm16 not 0 / 1; B outside 1..65535; negative in_start, n_in, m0 or len_host, n_out < 1; a stride
 * shorter than its row; a ratio whose tile of 256 outputs reads more than 16384 input samples (64 KiB of LDS); and any
 * requested output m < n_out(len_host) whose support within [0, len_host) is not inside [in_start, in_start + n_in).
 * Speed: tools/bench_resample.py. */
int fwn_resample_taps(int up, int down, int zeros);
int fwn_resample_design(int up, int down, int zeros, double beta, double rolloff, float* table_host);
int fwn_resample(const void* x, int x_pcm16, int64_t B, int64_t x_stride, int64_t in_start, int64_t n_in, const int64_t* len_dev,
                 int64_t len_host, const float* table_dev, int up, int down, int zeros, float* y, int64_t y_stride, int64_t m0,
                 int64_t n_out, void* stream);

/* ---- spectral denoiser (additive; FWN_VERSION unchanged): STFT, bias-spectrum subtraction and inverse STFT on the device, so
 * that synthesize --denoise keeps "only the mel goes up, only int16 comes down".  DESIGN.md 6b has the definition;
 * tests/denoise_ref.py restates it in fp64.
 *
 * n_fft a power of two in 32..4096, 1 <= hop <= n_fft / 2, w[n] = 0.5 - 0.5 cos(2 pi n / n_fft), nb = n_fft / 2 + 1.  A clip of
 * N samples has F = 1 + N div hop centred frames v_f[n] = w[n] x[j], j = f hop + n - n_fft / 2 reflected (j < 0 -> -j,
 * j >= N -> 2 (N - 1) - j) - fwn_mel_spectrogram's framing; X[f][k] = sum_n v_f[n] e^(-2 pi i k n / n_fft), k < nb;
 *     Y[f][k] = X[f][k] (1 - s b[k] / |X[f][k]|) where |X[f][k]| > s b[k], else 0          (s = strength, b = bias)
 *     out[n] = sum_f w[p - f hop] irfft(Y[f])[p - f hop] / sum_f w[p - f hop]^2,  p = n + n_fft / 2
 * both sums over the frames f <= F - 1 that cover p, in ascending f.  A clip of N < n_fft / 2 + 1 samples cannot be reflect-
 * padded and is returned unchanged.
 *
 * fwn_denoise: one launch for B clips, no workspace (fwn_denoise_workspace_bytes is 0; workspace may be NULL).  x: row b at
 * x + b * x_stride floats; clip b has N_b = len_dev[b] samples (DEVICE int64 [B], read on the device and clamped to
 * [0, len_host]) or len_host when len_dev is NULL.  y (float, may be NULL) and pcm (int16, may be NULL; not both): rows at
 * y + b * y_stride / pcm + b * pcm_stride; elements [0, len_host) of each row are written and nothing else: the result for
 * i < N_b, exact +0 / PCM 0 from N_b on.  pcm = fwn_pcm16's arithmetic on the float result, bit for bit.  No sample at or past
 * N_b is loaded.  A workgroup owns fwn_denoise_tile(n_fft, hop) consecutive samples and transforms the frames that cover them in
 * LDS; a frame is computed by the same instructions whichever tile computes it, so an output's bits depend on the clip's samples
 * within n_fft of it, on N_b, bias and strength only - not on B, the row, len_host or the tiling.  strength = 0 returns x to
 * rounding ((16 log2 n_fft + 16) 2^-24 relative to the frames' norms: DESIGN.md 6b).  Refusals (FWN_ERR_ARG, before any launch):
 * n_fft not a power of two in 32..4096; hop outside 1..n_fft/2; a null x, bias_dev or both outputs null; a pointer off its
 * element's alignment (len_dev: 8); B outside 1..65535; len_host outside 1..2^40; a stride shorter than len_host (or above 2^44); a negative,
 * infinite or NaN strength; a workspace smaller than fwn_denoise_workspace_bytes (or bytes at a null pointer); an output that
 * overlaps the input.
 *
 * fwn_stft_mean_mag: mag_out[k] (DEVICE float [nb]) = the mean over the interior frames - those whose n_fft samples lie inside
 * the clip: ceil(n_fft / 2 / hop) <= f <= (len_host - n_fft / 2) div hop - of the B rows (each len_host long) of |X[f][k]|,
 * summed per bin in fp64 in frame order by one workgroup: the model's bias from a clip synthesized from nothing.  Refuses what
 * fwn_denoise refuses of these arguments, a clip with no interior frame, and more than 2^20 interior frames in all.
 * Speed: tools/bench_denoise.py. */
int fwn_denoise_tile(int n_fft, int hop);
size_t fwn_denoise_workspace_bytes(int64_t B, int64_t len_host, int n_fft, int hop);
int fwn_stft_mean_mag(const float* x, int64_t B, int64_t x_stride, int64_t len_host, int n_fft, int hop, float* mag_out, void* stream);
int fwn_denoise(const float* x, int64_t B, int64_t x_stride, const int64_t* len_dev, int64_t len_host, const float* bias_dev,
                float strength, int n_fft, int hop, float* y, int64_t y_stride, int16_t* pcm, int64_t pcm_stride, void* workspace,
                size_t workspace_bytes, void* stream);

/* ---- ragged mel front-end (additive; FWN_VERSION unchanged): peak normalisation, the log-mel spectrogram through the denoiser's
 * LDS FFT and the reference's centre-padded audio for B clips of different lengths, in two launches.  DESIGN.md 6c has the
 * definition; tests/mel_front_ref.py restates it.  fwn_mel_spectrogram (one rectangle, direct DFT) is untouched.
 *
 * Framing as above: n_fft a power of two in 32..4096, 1 <= hop <= n_fft / 2, nb = n_fft / 2 + 1, a clip of N samples has
 * F = 1 + N div hop centred, reflect-padded frames under the periodic Hann window.  x: row b at x + b * x_stride floats; clip b
 * has N_b = len_dev[b] samples (DEVICE int64 [B], read on the device and clamped to [0, len_host]) or len_host when len_dev is
 * NULL; no sample at or past N_b is loaded.  F_host = 1 + len_host div hop.
 *
 * fwn_clip_peak: peak_out[b] (DEVICE float [B]) = max_{i < N_b} |x[i]|: +0 for an empty clip, NaN if any sample is NaN, else
 * exact (an integer maximum over the bit patterns: the result does not depend on B, the row, the stride or the order).  A clip
 * is split over workgroups of 16384 samples; the output need not be cleared (a memset node precedes the one launch).
 *
 * fwn_mel_front: one launch, no workspace.  xn[i] = (x[i] / peak_dev[b]) * rmax - two separately rounded fp32 operations, the
 * division IEEE: the float32 arithmetic of the reference's wav / max|wav| * rescaling_max - or xn = x when peak_dev is NULL.
 *     P[f][m] = sum_k fb[m][k] |X_f[k]|^2 (ascending k, fmaf), X_f the transform of frame f of xn,
 *     mel[f][m] = clip((20 log10(max(1e-4, P[f][m])) - ref_level_db - min_level_db) / -min_level_db, 0, 1)
 * fb: DEVICE float [n_mels][nb], dense.  bands (DEVICE int32 [n_mels][2], may be NULL): first and one-past-last non-zero bin of
 * each row of fb; it restricts the k loop and, for finite input, changes no bit (a skipped term is fmaf(0, p, acc) = acc).
 * mel: row b at mel + b * mel_stride floats, [F_host][n_mels]: rows f < F_b hold the result, rows F_b <= f < F_host exact +0.
 * audio (may be NULL): row b at audio + b * audio_stride floats, F_host * hop samples: audio[i] = xn[i - pad_l] for
 * pad_l <= i < pad_l + N_b, pad_l = (F_b hop - N_b) div 2, and +0 elsewhere - the reference's padded, trimmed clip.  Nothing else
 * is written.  A clip whose peak is not > 0 (silent, NaN) or with N_b < n_fft / 2 + 1 (cannot be reflected) gets all-zero mel
 * and audio rows.  A workgroup owns fwn_mel_front_frames(n_fft, hop) consecutive frames of one clip; a frame is computed by the
 * same instructions wherever it lands, so mel[f]'s bits depend on the clip's samples in the frame's support, on N_b, peak[b],
 * rmax and fb only - not on B, the row, len_host or the grid.  Error against fp64: tests/mel_front_ref.py bound().
 * Refusals (FWN_ERR_ARG, before any launch): n_fft not a power of two in 32..4096; hop outside 1..n_fft/2; a null x, fb, mel or
 * peak_out; a pointer off its element's alignment (len_dev: 8); B outside 1..65535; len_host outside 1..2^40; a stride shorter
 * than the row it holds (or above 2^44); min_level_db >= 0; a non-finite rmax, or rmax <= 0 with peak_dev; n_mels outside
 * 1..1024; more than 2^31 - 1 workgroups per row; an output that overlaps the input.
 * Speed: tools/bench_mel.py. */
int fwn_mel_front_frames(int n_fft, int hop);
int fwn_clip_peak(const float* x, int64_t B, int64_t x_stride, const int64_t* len_dev, int64_t len_host, float* peak_out, void* stream);
int fwn_mel_front(const float* x, int64_t B, int64_t x_stride, const int64_t* len_dev, int64_t len_host, const float* peak_dev, float rmax,
                  const float* fb, const int32_t* bands, int n_fft, int hop, int n_mels, float ref_level_db, float min_level_db, float* mel,
                  int64_t mel_stride, float* audio, int64_t audio_stride, void* stream);

/* ---- spectral distances (additive; FWN_VERSION unchanged): how close a test clip is to its target - mel L1, log-spectral
 * distance and spectral convergence of B pairs of clips of different lengths, through the same LDS FFT, in two launches; no
 * spectrogram is written to memory and four doubles per pair come out.  DESIGN.md 6d has the definition; tests/specdist_ref.py
 * restates it in fp64.
 *
 * Framing as above: n_fft a power of two in 32..4096, 1 <= hop <= n_fft / 2, nb = n_fft / 2 + 1.  Pair b is x (the target), row b
 * at x + b * x_stride floats, and y (the test), row b at y + b * y_stride floats, both of N_b = len_dev[b] samples (DEVICE int64
 * [B], read on the device and clamped to [0, len_host]) or len_host when len_dev is NULL; no sample at or past N_b is loaded; x
 * and y are only read and may overlap each other.  F_b = 1 + N_b div hop frames; X_f, Y_f the transforms of frame f; Px = |X|^2,
 * Py = |Y|^2 in fp32 as fwn_mel_front forms them.
 *     mel_l1 = mean_{f < F_b, m < n_mels} |mel_x[f][m] - mel_y[f][m]|, mel_* being fwn_mel_front's mel with peak_dev NULL - the
 *              same filter loop over fb (and bands), dB and clip: the distance in the space the model is conditioned on, in
 *              fractions of -min_level_db.  NaN when fb is NULL (n_mels, bands and the dB constants are then unused).
 *     lsd_db = mean_f sqrt( mean_{k < nb} (10 log10 max(floor, Px) - 10 log10 max(floor, Py))^2 )
 *     sc     = sqrt( sum_{f,k} (sqrt Px - sqrt Py)^2 ) / sqrt( sum_{f,k} Px );  the IEEE quotient when the target's spectrum is
 *              all zero: NaN for 0 / 0, +inf otherwise
 * The terms are fp32, every sum fp64.  out: DEVICE double [B][4] = mel_l1, lsd_db, sc, F_b.  A pair with N_b < n_fft / 2 + 1
 * cannot be reflected: NaN, NaN, NaN, 0.  Nothing else is written but the workspace.
 *
 * First launch: a workgroup owns fwn_spectral_distance_frames(n_fft, hop) consecutive frames of one pair, transforms frame f of
 * x and of y (side by side; one after the other at n_fft 2048 and 4096), adds the terms with lanes on fixed bins through a fixed
 * shuffle-and-LDS tree, and stores four partials (sum |dmel|, sum_f lsd_f, sum (|X| - |Y|)^2, sum |X|^2) at [b][workgroup] of
 * the workspace (fwn_spectral_distance_workspace_bytes: B * ceil(F_host / frames) * 32, F_host = 1 + len_host div hop; 0 for
 * arguments fwn_spectral_distance refuses; need not be cleared).  Second launch: one wave per pair adds the partials
 * 0 .. ceil(F_b / frames) - 1 in an order that F_b alone decides, divides and takes the roots.  No atomics, no synchronisation
 * with the host.  A pair's four doubles depend on its two sets of samples, N_b, fb, the dB constants and floor only - not on B,
 * the row, the strides, len_host, the grid or bands (for finite input a skipped term is fmaf(0, p, acc) = acc).
 * Error against fp64: tests/specdist_ref.py bound().
 * Refusals (FWN_ERR_ARG, before any launch): n_fft not a power of two in 32..4096; hop outside 1..n_fft/2; a null x, y or out; a
 * pointer off its element's alignment (len_dev, out, workspace: 8); B outside 1..65535; len_host outside 1..2^40; a stride
 * shorter than len_host (or above 2^44); with fb: n_mels outside 1..1024, min_level_db >= 0; bands without fb; a floor that is
 * not finite or not > 0; a null workspace or one smaller than fwn_spectral_distance_workspace_bytes; out or the workspace
 * overlapping an input or each other; more than 2^31 - 1 workgroups per row.
 * Speed: tools/bench_specdist.py. */
int fwn_spectral_distance_frames(int n_fft, int hop);
size_t fwn_spectral_distance_workspace_bytes(int64_t B, int64_t len_host, int n_fft, int hop);
int fwn_spectral_distance(const float* x, int64_t x_stride, const float* y, int64_t y_stride, int64_t B, const int64_t* len_dev,
                          int64_t len_host, const float* fb, const int32_t* bands, int n_fft, int hop, int n_mels, float ref_level_db,
                          float min_level_db, float floor, double* out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FWN_H */
