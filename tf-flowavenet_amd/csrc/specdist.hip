// Spectral distances of B pairs of clips (include/fwn.h "spectral distances"; DESIGN.md 6d has the definition): per pair the mel
// L1 in the front-end's own log-mel space, the log-spectral distance and the spectral convergence, through the LDS FFT of
// stft_lds.h - two launches, no atomics, no spectrogram in HBM, four doubles per clip out.
//   specdist_kernel        a workgroup owns FRAMES consecutive frames of one pair and transforms frame f of x and of y: side by side
//                          in slots 2p, 2p + 1 where batch_of(n_fft) >= 2, one after the other at n_fft 2048 and 4096 (one slot:
//                          x's power row waits in the tail, y's goes to the ping-pong buffer the passes left free).
//     load, forward, power   stft_lds.h's load_frame, fft_passes and power_rows, the ones melfront.hip calls (peak NULL), so a
//                            frame's power row has the front-end's bits
//     per bin  (10 log10 max(floor, Px) - 10 log10 max(floor, Py))^2, (sqrt Px - sqrt Py)^2 and Px in fp32, added in fp64 by the
//              lane that owns bins tid, tid + NT, ...
//     per mel  stft_lds.h's mel_of, the front-end's, for x and for y, |difference| in fp32, added in fp64 by the lane that owns
//              (pair, mel)
//     sums     a butterfly over the wave, the four waves' values through LDS and added in order by lane 0; a frame's lsd is rooted
//              there and added to the workgroup's in frame order
//   and stores its four partials at [b][workgroup] of the workspace.  Workgroups at or past the clip's own frames return at once.
//   specdist_final_kernel  one wave per clip adds the partials 0 .. ceil(F_b / FRAMES) - 1 - lane l takes l, l + 64, ... in order,
//                          then the butterfly -, divides, takes the roots and writes out[b].
// Which lane adds what, and in which order, follows from n_fft, n_mels and F_b alone: a clip's four doubles depend on its two
// sets of samples, N_b, fb, the dB constants and floor only.  The argument checks are audio_args.h's.
#include "audio_args.h"
#include "row_steps.h"
#include "stft_lds.h"

namespace {

using namespace stft_lds;
using namespace audio_args;

constexpr int FRAMES = 8;                   // frames of a pair a workgroup owns (fwn_spectral_distance_frames): a multiple of every G / 2
constexpr int MAXP = 4;                     // pairs side by side at most: batch_of() / 2
constexpr int NW = NT / 64;

// v[i] summed over the workgroup, in lane 0 of wave 0 (every lane of a wave holds its wave's sum): the same tree every time
template <int n>
__device__ __forceinline__ void block_sum(double (&v)[n], double (*red)[MAXP]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < n; ++i) {
        for (int d = 32; d >= 1; d >>= 1) v[i] += __shfl_xor(v[i], d, 64);
        if ((tid & 63) == 0) red[tid >> 6][i] = v[i];
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < n; ++i) {
            double s = red[0][i];
            for (int w = 1; w < NW; ++w) s += red[w][i];
            v[i] = s;
        }
    }
    __syncthreads();                                           // red, and whatever LDS the caller read, may be written again
}

__global__ __launch_bounds__(NT) void specdist_kernel(const float* x, long x_stride, const float* y, long y_stride,
                                                      const long long* __restrict__ len_dev, long len_host, const float* __restrict__ fb,
                                                      const int* __restrict__ bands, int n_fft, int lognc, int hop, int n_mels, int G,
                                                      float ref_db, float min_db, float floor, double* __restrict__ part, long groups) {
    extern __shared__ float sm[];
    __shared__ double red[NW][MAXP];
    const int tid = threadIdx.x, h = n_fft / 2, nc = h, nb = h + 1;
    const long b = blockIdx.y;
    const long N = clamp_len(len_dev, b, len_host);
    const long F = 1 + N / hop;
    const long f0 = (long)blockIdx.x * FRAMES;
    if (N < h + 1 || f0 >= F) return;                          // too short to reflect, or past the clip: nothing that is read later
    const int nf = F - f0 < FRAMES ? (int)(F - f0) : FRAMES;
    const float* xrow = x + b * x_stride;
    const float* yrow = y + b * y_stride;

    Lds l = carve(sm, n_fft, G);
    float* pw = l.tail;                                        // [G][nb] power rows: x of pair p in 2p, y in 2p + 1
    fill_twiddles(l.tw, n_fft);
    __syncthreads();
    const int P = G >= 2 ? G / 2 : 1;                          // pairs per round
    double acc[3] = {0.0, 0.0, 0.0};                           // this lane's sum |dmel|, sum (|X| - |Y|)^2, sum |X|^2
    double lsd_sum = 0.0;                                      // lane 0: sum over the frames of lsd_f
    for (int g0 = 0; g0 < nf; g0 += P) {
        const int pairs = nf - g0 < P ? nf - g0 : P;
        const float* py_rows;                                  // y's row of pair p at py_rows + p * 2 nb, x's at pw + p * 2 nb
        if (G >= 2) {
            for (int p = 0; p < pairs; ++p) {
                load_frame(xrow, N, f0 + g0 + p, hop, n_fft, l.tw, (float*)(l.a + (size_t)(2 * p) * nc));
                load_frame(yrow, N, f0 + g0 + p, hop, n_fft, l.tw, (float*)(l.a + (size_t)(2 * p + 1) * nc));
            }
            __syncthreads();
            float2 *a = l.a, *bb = l.b;
            fft_passes(a, bb, l.tw, nc, lognc, 2 * pairs, -1.0f);
            power_rows(a, l.tw, 2 * pairs, nc, pw, nb);
            py_rows = pw + nb;
        } else {                                               // one slot: x, then y
            load_frame(xrow, N, f0 + g0, hop, n_fft, l.tw, (float*)l.a);
            __syncthreads();
            float2 *a = l.a, *bb = l.b;
            fft_passes(a, bb, l.tw, nc, lognc, 1, -1.0f);
            power_rows(a, l.tw, 1, nc, pw, nb);
            __syncthreads();                                   // x's power row is whole before l.a is loaded again
            load_frame(yrow, N, f0 + g0, hop, n_fft, l.tw, (float*)l.a);
            __syncthreads();
            a = l.a, bb = l.b;
            fft_passes(a, bb, l.tw, nc, lognc, 1, -1.0f);
            power_rows(a, l.tw, 1, nc, (float*)bb, nb);        // bb: the buffer the last pass read, free now; n_fft >= nb floats
            py_rows = (const float*)bb;
        }
        __syncthreads();

        double lsd[MAXP] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int p = 0; p < MAXP; ++p) {
            if (p < pairs) {
                const float* px_row = pw + (size_t)p * 2 * nb;
                const float* py_row = py_rows + (size_t)p * 2 * nb;
                for (int k = tid; k < nb; k += NT) {           // lane owns bins tid, tid + NT, ... of every frame
                    const float px = px_row[k], py = py_row[k];
                    const float dl = 10.0f * log10f(fmaxf(floor, px)) - 10.0f * log10f(fmaxf(floor, py));
                    const float dm = sqrtf(px) - sqrtf(py);
                    lsd[p] += (double)(dl * dl);
                    acc[1] += (double)(dm * dm);
                    acc[2] += (double)px;
                }
            }
        }
        if (fb) {
            for (int i = tid; i < pairs * n_mels; i += NT) {   // lane owns (pair p, mel m)
                const int p = i / n_mels, m = i - p * n_mels;
                const float mx = mel_of(fb, bands, m, nb, pw + (size_t)p * 2 * nb, ref_db, min_db);
                const float my = mel_of(fb, bands, m, nb, py_rows + (size_t)p * 2 * nb, ref_db, min_db);
                acc[0] += (double)fabsf(mx - my);
            }
        }
        block_sum(lsd, red);                                   // ends with a barrier: the next round may load over l.a and pw
        if (tid == 0)
            for (int p = 0; p < pairs; ++p) lsd_sum += sqrt(lsd[p] / (double)nb);
    }
    block_sum(acc, red);
    if (tid == 0) {
        double* o = part + ((size_t)b * groups + blockIdx.x) * 4;
        o[0] = acc[0];
        o[1] = lsd_sum;
        o[2] = acc[1];
        o[3] = acc[2];
    }
}

__global__ __launch_bounds__(64) void specdist_final_kernel(const double* __restrict__ part, long groups, const long long* __restrict__ len_dev,
                                                            long len_host, int n_fft, int hop, int n_mels, int has_fb,
                                                            double* __restrict__ out) {
    const int lane = threadIdx.x;
    const long b = blockIdx.x;
    const long N = clamp_len(len_dev, b, len_host);
    double* o = out + b * 4;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (N < n_fft / 2 + 1) {                                   // cannot be reflected: no frame, no measure
        if (lane == 0) { o[0] = nan; o[1] = nan; o[2] = nan; o[3] = 0.0; }
        return;
    }
    const long F = 1 + N / hop, ng = (F + FRAMES - 1) / FRAMES;
    const double* p = part + (size_t)b * groups * 4;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long g = lane; g < ng; g += 64)
        for (int i = 0; i < 4; ++i) s[i] += p[g * 4 + i];
    for (int i = 0; i < 4; ++i)
        for (int d = 32; d >= 1; d >>= 1) s[i] += __shfl_xor(s[i], d, 64);
    if (lane == 0) {
        o[0] = has_fb ? s[0] / ((double)F * (double)n_mels) : nan;
        o[1] = s[1] / (double)F;
        o[2] = sqrt(s[2]) / sqrt(s[3]);                        // IEEE when the target is silent: NaN for 0 / 0, +inf otherwise
        o[3] = (double)F;
    }
}

int64_t groups_of(int64_t len_host, int hop) { return (1 + len_host / hop + FRAMES - 1) / FRAMES; }

}  // namespace

extern "C" {

int fwn_spectral_distance_frames(int n_fft, int hop) {
    if (int rc = check_shape("fwn_spectral_distance_frames", n_fft, hop)) return rc;
    return FRAMES;
}

size_t fwn_spectral_distance_workspace_bytes(int64_t B, int64_t len_host, int n_fft, int hop) {
    if (check_shape("fwn_spectral_distance_workspace_bytes", n_fft, hop) || B < 1 || B >= 65536 || len_host < 1 || len_host > MAX_LEN) return 0;
    return (size_t)B * (size_t)groups_of(len_host, hop) * 4 * sizeof(double);
}

int fwn_spectral_distance(const float* x, int64_t x_stride, const float* y, int64_t y_stride, int64_t B, const int64_t* len_dev,
                          int64_t len_host, const float* fb, const int32_t* bands, int n_fft, int hop, int n_mels, float ref_level_db,
                          float min_level_db, float floor, double* out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "fwn_spectral_distance";
    if (int rc = check_shape(fn, n_fft, hop)) return rc;
    if (int rc = check_clips(fn, B, len_dev, len_host)) return rc;
    if (int rc = check_rows(fn, "x", x, 4, x_stride, len_host)) return rc;
    if (int rc = check_rows(fn, "y", y, 4, y_stride, len_host)) return rc;
    if (int rc = check_ptr(fn, "out", out, 8)) return rc;
    if (int rc = check_ptr(fn, "fb", fb, 4, true)) return rc;
    if (int rc = check_ptr(fn, "bands", bands, 4, true)) return rc;
    if (int rc = check_ptr(fn, "workspace", workspace, 8, true)) return rc;
    AREQUIRE(fb || !bands, "%s: bands without fb", fn);
    AREQUIRE(!fb || (n_mels >= 1 && n_mels <= 1024), "%s: n_mels %d outside 1..1024", fn, n_mels);
    AREQUIRE(!fb || min_level_db < 0.0f, "%s: min_level_db %g must be negative", fn, (double)min_level_db);
    AREQUIRE(floor > 0.0f && floor <= 3.0e38f, "%s: floor %g is not a finite positive power", fn, (double)floor);
    const int64_t groups = groups_of(len_host, hop);
    AREQUIRE(groups < ((int64_t)1 << 31), "%s: %lld workgroups per row, past 2^31 - 1", fn, (long long)groups);
    const size_t need = (size_t)B * (size_t)groups * 4 * sizeof(double);
    AREQUIRE(workspace && workspace_bytes >= need, "%s: workspace of %zu bytes is null or smaller than the %zu of fwn_spectral_distance_workspace_bytes",
             fn, workspace_bytes, need);
    const int64_t xb = ((B - 1) * x_stride + len_host) * 4, yb = ((B - 1) * y_stride + len_host) * 4, ob = B * 4 * (int64_t)sizeof(double);
    AREQUIRE(!overlap(x, xb, out, ob) && !overlap(y, yb, out, ob) && !overlap(x, xb, workspace, (int64_t)need) &&
             !overlap(y, yb, workspace, (int64_t)need) && !overlap(out, ob, workspace, (int64_t)need),
             "%s: out or the workspace overlaps an input, or each other", fn);
    const int G = batch_of(n_fft);
    const size_t lds = lds_floats(n_fft, G) * sizeof(float);  // 57 352 bytes at n_fft 4096: under the 64 KiB a launch gets unasked
    hipLaunchKernelGGL(specdist_kernel, dim3((unsigned)groups, (unsigned)B), dim3(NT), lds, (hipStream_t)stream, x, (long)x_stride, y,
                       (long)y_stride, (const long long*)len_dev, (long)len_host, fb, (const int*)bands, n_fft, log2_of(n_fft / 2), hop,
                       n_mels, G, ref_level_db, min_level_db, floor, (double*)workspace, (long)groups);
    if (int rc = launched(fn)) return rc;
    hipLaunchKernelGGL(specdist_final_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, (long)groups,
                       (const long long*)len_dev, (long)len_host, n_fft, hop, n_mels, fb ? 1 : 0, out);
    return launched(fn);
}

}  // extern "C"
