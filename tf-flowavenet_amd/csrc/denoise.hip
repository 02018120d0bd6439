// Spectral denoiser (include/fwn.h "spectral denoiser"; DESIGN.md 6b has the definition): centred reflect-padded STFT with the
// periodic Hann window, soft threshold of every bin's magnitude by strength * bias[k] with the phase kept, inverse STFT by
// least-squares overlap-add.  One launch: a workgroup owns TILE consecutive output samples of one clip and walks the frames
// that cover them in ascending order, G at a time:
//   load     v_f[n] = w[n] x[reflect(f hop + n - n_fft / 2)] as n_fft / 2 complex points z[m] = v[2m] + i v[2m + 1]
//   forward  radix-2 Stockham passes over the nc = n_fft / 2 complex points, ping-pong between two LDS buffers
//   split    X[k], X[nc - k] from Z[k], Z[nc - k]; the threshold; and back to the Z' whose inverse transform is irfft(Y) - in place
//   inverse  the same passes with conjugate twiddles (the 1 / n_fft is folded, exactly, into the split)
//   add      lane t owns tile samples t, t + 256, ...: acc += w[n] y_f[n] in registers, frames in ascending f
// and at the end divides by the envelope sum_f w^2 (same frames, same order).  A frame is computed by the same instructions
// whichever tile, batch slot or row computes it, and a sample's sums run over its covering frames in ascending f, so an output's
// bits depend on the clip's samples within n_fft of it, the clip's length, bias and strength only.  Twiddles come from
// sincospif once per workgroup; the window is 0.5 - 0.5 cos from the same table.  mean_mag_kernel is the bias: the forward
// half over the interior frames of B equal rows, |X[k]| summed per bin in fp64 in frame order by one workgroup.
// The load, the passes and the split are stft_lds.h's (shared with melfront.hip and specdist.hip); its header has the LDS bank
// notes.  The PCM sample is row_steps.h's pcm16_of, fwn_pcm16's own; the argument checks are audio_args.h's.
#include "audio_args.h"
#include "row_steps.h"
#include "stft_lds.h"

namespace {

using namespace stft_lds;                   // NT, batch_of, lds_floats: [n_fft / 2 + 1] thresholds (or, for the bias, fp64 sums) in the tail
using namespace audio_args;

constexpr int TILE = 2048;                  // output samples per workgroup
constexpr int PER = TILE / NT;              // samples a lane owns: tile samples lane, lane + NT, ...
constexpr int64_t MAX_BIAS_FRAMES = 1 << 20;

// soft threshold of the magnitude, the phase kept: X (1 - t / |X|) where |X| > t, else 0.  t = 0 returns X's own bits.
__device__ __forceinline__ float2 shrink(float2 X, float t) {
    const float mag = sqrtf(X.x * X.x + X.y * X.y);
    const float g = mag > t ? 1.0f - t / mag : 0.0f;
    return make_float2(X.x * g, X.y * g);
}
__device__ __forceinline__ float shrink_real(float X, float t) {
    const float mag = fabsf(X);
    return X * (mag > t ? 1.0f - t / mag : 0.0f);
}

// Z (the forward transform of `frames` slots) -> Z' in place: irfft(Y)[2m] + i irfft(Y)[2m + 1] = IFFT_unscaled(Z')[m].
// One lane per pair (k, nc - k), k = 0 .. nc / 2; sb[k] = strength * bias[k]; sc = 1 / n_fft.
__device__ __forceinline__ void threshold_in_place(float2* z, const float2* tw, const float* sb, int nc, int frames, float sc) {
    const int half = nc >> 1, per = half + 1;
    for (int i = threadIdx.x; i < frames * per; i += NT) {
        const int g = i / per, k = i - g * per;
        float2* zf = z + (size_t)g * nc;
        if (k == 0) {                                          // X[0] and X[nc] are real
            const float2 A = zf[0];
            const float y0 = shrink_real(A.x + A.y, sb[0]), yn = shrink_real(A.x - A.y, sb[nc]);
            zf[0] = make_float2((y0 + yn) * sc, (y0 - yn) * sc);
        } else if (k == half) {                                // its own partner: X = conj Z, Z' = 2 conj Y
            const float2 A = zf[half];
            const float2 Y = shrink(make_float2(A.x, -A.y), sb[half]);
            zf[half] = make_float2(2.0f * sc * Y.x, -(2.0f * sc * Y.y));
        } else {
            const float2 w = tw[k];
            float2 Xk, Xm;
            split_pair(zf[k], zf[nc - k], w, Xk, Xm);
            const float2 Yk = shrink(Xk, sb[k]), Ym = shrink(Xm, sb[nc - k]);
            const float pr = Yk.x + Ym.x, pi = Yk.y - Ym.y;    // Y[k] + conj Y[nc - k]
            const float qr = Yk.x - Ym.x, qi = Yk.y + Ym.y;    // Y[k] - conj Y[nc - k]
            const float or_ = qr * w.x - qi * w.y, oi = qr * w.y + qi * w.x;       // times e^(+2 pi i k / n_fft)
            zf[k] = make_float2((pr - oi) * sc, (pi + or_) * sc);
            zf[nc - k] = make_float2((pr + oi) * sc, (or_ - pi) * sc);
        }
    }
}

__device__ __forceinline__ void put(float* yrow, short* prow, long i, float v) {
    if (yrow) yrow[i] = v;
    if (prow) prow[i] = pcm16_of(v);
}

__global__ __launch_bounds__(NT) void denoise_kernel(const float* __restrict__ x, long x_stride, const long long* __restrict__ len_dev,
                                                     long len_host, const float* __restrict__ bias, float strength, int n_fft,
                                                     int lognc, int hop, int G, float* __restrict__ y, long y_stride,
                                                     short* __restrict__ pcm, long pcm_stride) {
    extern __shared__ float sm[];
    const int tid = threadIdx.x, h = n_fft / 2, nc = h;
    const long b = blockIdx.y;
    const long N = clamp_len(len_dev, b, len_host);
    const long t0 = (long)blockIdx.x * TILE;                   // first sample of this tile
    const long left = len_host - t0;
    const int cnt = left < TILE ? (int)left : TILE;            // the row's samples in it: what this workgroup writes
    const float* xrow = x + b * x_stride;
    float* yrow = y ? y + b * y_stride : nullptr;
    short* prow = pcm ? pcm + b * pcm_stride : nullptr;
    if (t0 >= N || N < h + 1) {                                // past the clip: +0; a clip too short to reflect-pad: itself
        for (int s = tid; s < cnt; s += NT) put(yrow, prow, t0 + s, t0 + s < N ? xrow[t0 + s] : 0.0f);
        return;
    }
    const long F = 1 + N / hop;
    const int nv = N - t0 < cnt ? (int)(N - t0) : cnt;         // the clip's samples in the tile, >= 1
    // the frames f <= F - 1 with f hop <= p < f hop + n_fft for some p = sample + h of the tile
    const long p_lo = t0 + h, p_hi = t0 + nv - 1 + h;
    const long f_lo = p_lo - n_fft + 1 <= 0 ? 0 : (p_lo - n_fft + hop) / hop;
    const long f_hi = p_hi / hop < F - 1 ? p_hi / hop : F - 1;

    Lds l = carve(sm, n_fft, G);
    float* sb = l.tail;                                        // [nc + 1] strength * bias
    fill_twiddles(l.tw, n_fft);
    for (int k = tid; k <= nc; k += NT) sb[k] = strength * bias[k];
    __syncthreads();

    float acc[PER];
    for (int r = 0; r < PER; ++r) acc[r] = 0.0f;
    const float sc = 1.0f / (float)n_fft;
    for (long g0 = f_lo; g0 <= f_hi; g0 += G) {
        const int frames = f_hi - g0 + 1 < G ? (int)(f_hi - g0 + 1) : G;
        for (int g = 0; g < frames; ++g) load_frame(xrow, N, g0 + g, hop, n_fft, l.tw, (float*)(l.a + (size_t)g * nc));
        __syncthreads();
        float2 *a = l.a, *bb = l.b;
        fft_passes(a, bb, l.tw, nc, lognc, frames, -1.0f);
        threshold_in_place(a, l.tw, sb, nc, frames, sc);
        __syncthreads();
        fft_passes(a, bb, l.tw, nc, lognc, frames, 1.0f);      // 2 lognc passes in all: the result is in l.a
        const float* yf = (const float*)l.a;
        for (int r = 0; r < PER; ++r) {
            const int s = tid + NT * r;
            if (s >= nv) continue;
            const long p = t0 + s + h;
            for (int g = 0; g < frames; ++g) {
                const long n = p - (g0 + g) * hop;
                if (n >= 0 && n < n_fft) acc[r] += hann(l.tw, (int)n, h) * yf[(size_t)g * n_fft + n];
            }
        }
        __syncthreads();                                       // before the next batch is loaded over l.a
    }
    for (int r = 0; r < PER; ++r) {
        const int s = tid + NT * r;
        if (s >= cnt) continue;
        float v = 0.0f;
        if (s < nv) {
            const long p = t0 + s + h;
            const long fa = p - n_fft + 1 <= 0 ? 0 : (p - n_fft + hop) / hop;
            const long fb = p / hop < F - 1 ? p / hop : F - 1;
            float env = 0.0f;
            for (long f = fa; f <= fb; ++f) {
                const float w = hann(l.tw, (int)(p - f * hop), h);
                env += w * w;
            }
            v = acc[r] / env;
        }
        put(yrow, prow, t0 + s, v);
    }
}

// mag_out[k] = mean over the B rows' interior frames (f_min .. f_min + n_int - 1, rows in order) of |X[f, k]|: one workgroup,
// the sums in fp64 in LDS, every bin owned by one lane.
__global__ __launch_bounds__(NT) void mean_mag_kernel(const float* __restrict__ x, long B, long x_stride, long N, int n_fft, int lognc,
                                                      int hop, int G, long f_min, long n_int, float* __restrict__ mag_out) {
    extern __shared__ float sm[];
    const int tid = threadIdx.x, h = n_fft / 2, nc = h, half = nc >> 1, per = half + 1;
    Lds l = carve(sm, n_fft, G);
    double* sum = (double*)l.tail;                             // [nc + 1]; the carve keeps it 8-byte aligned
    fill_twiddles(l.tw, n_fft);
    for (int k = tid; k <= nc; k += NT) sum[k] = 0.0;
    __syncthreads();
    const long total = B * n_int;
    for (long q0 = 0; q0 < total; q0 += G) {
        const int frames = total - q0 < G ? (int)(total - q0) : G;
        for (int g = 0; g < frames; ++g) {
            const long q = q0 + g, row = q / n_int;
            load_frame(x + row * x_stride, N, f_min + (q - row * n_int), hop, n_fft, l.tw, (float*)(l.a + (size_t)g * nc));
        }
        __syncthreads();
        float2 *a = l.a, *bb = l.b;
        fft_passes(a, bb, l.tw, nc, lognc, frames, -1.0f);
        for (int k = tid; k < per; k += NT)                    // lane owns bins k and nc - k; frames in order
            for (int g = 0; g < frames; ++g) {
                const float2* zf = a + (size_t)g * nc;
                if (k == 0) {
                    sum[0] += (double)fabsf(zf[0].x + zf[0].y);
                    sum[nc] += (double)fabsf(zf[0].x - zf[0].y);
                } else if (k == half) {
                    sum[half] += (double)sqrtf(zf[half].x * zf[half].x + zf[half].y * zf[half].y);
                } else {
                    float2 Xk, Xm;
                    split_pair(zf[k], zf[nc - k], l.tw[k], Xk, Xm);
                    sum[k] += (double)sqrtf(Xk.x * Xk.x + Xk.y * Xk.y);
                    sum[nc - k] += (double)sqrtf(Xm.x * Xm.x + Xm.y * Xm.y);
                }
            }
        __syncthreads();
    }
    for (int k = tid; k <= nc; k += NT) mag_out[k] = (float)(sum[k] / (double)total);
}

}  // namespace

extern "C" {

int fwn_denoise_tile(int n_fft, int hop) {
    if (int rc = check_shape("fwn_denoise_tile", n_fft, hop)) return rc;
    return TILE;
}

size_t fwn_denoise_workspace_bytes(int64_t B, int64_t len_host, int n_fft, int hop) {
    (void)B; (void)len_host; (void)n_fft; (void)hop;
    return 0;                                                  // the fused form keeps every frame in LDS
}

int fwn_stft_mean_mag(const float* x, int64_t B, int64_t x_stride, int64_t len_host, int n_fft, int hop, float* mag_out, void* stream) {
    const char* fn = "fwn_stft_mean_mag";
    if (int rc = check_shape(fn, n_fft, hop)) return rc;
    if (int rc = check_clips(fn, B, nullptr, len_host)) return rc;
    if (int rc = check_rows(fn, "x", x, 4, x_stride, len_host)) return rc;
    if (int rc = check_ptr(fn, "mag_out", mag_out, 4)) return rc;
    // interior: the frame's n_fft samples [f hop - n_fft / 2, f hop + n_fft / 2) lie inside [0, len_host)
    const int64_t h = n_fft / 2, f_min = (h + hop - 1) / hop, f_max = (len_host - h) / hop;
    AREQUIRE(len_host >= n_fft && f_max >= f_min, "%s: a clip of %lld samples has no interior frame at n_fft %d, hop %d", fn,
             (long long)len_host, n_fft, hop);
    const int64_t n_int = f_max - f_min + 1;
    AREQUIRE(B * n_int <= MAX_BIAS_FRAMES, "%s: %lld interior frames, more than the %lld one workgroup is given", fn,
             (long long)(B * n_int), (long long)MAX_BIAS_FRAMES);
    const int G = batch_of(n_fft);
    hipLaunchKernelGGL(mean_mag_kernel, dim3(1), dim3(NT), lds_floats(n_fft, 2) * sizeof(float), (hipStream_t)stream, x, (long)B,
                       (long)x_stride, (long)len_host, n_fft, log2_of(n_fft / 2), hop, G, (long)f_min, (long)n_int, mag_out);
    return launched(fn);
}

int fwn_denoise(const float* x, int64_t B, int64_t x_stride, const int64_t* len_dev, int64_t len_host, const float* bias_dev,
                float strength, int n_fft, int hop, float* y, int64_t y_stride, int16_t* pcm, int64_t pcm_stride, void* workspace,
                size_t workspace_bytes, void* stream) {
    const char* fn = "fwn_denoise";
    if (int rc = check_shape(fn, n_fft, hop)) return rc;
    if (int rc = check_clips(fn, B, len_dev, len_host)) return rc;
    if (int rc = check_rows(fn, "x", x, 4, x_stride, len_host)) return rc;
    if (int rc = check_ptr(fn, "bias_dev", bias_dev, 4)) return rc;
    AREQUIRE(y || pcm, "%s: null pointer (both outputs)", fn);
    if (y) if (int rc = check_rows(fn, "y", y, 4, y_stride, len_host)) return rc;
    if (pcm) if (int rc = check_rows(fn, "pcm", pcm, 2, pcm_stride, len_host)) return rc;
    AREQUIRE(strength >= 0.0f && strength <= 3.0e38f, "%s: strength %g is negative, infinite or NaN", fn, (double)strength);
    AREQUIRE(workspace_bytes >= fwn_denoise_workspace_bytes(B, len_host, n_fft, hop) && (workspace || workspace_bytes == 0),
             "%s: workspace of %zu bytes at a null pointer, or smaller than fwn_denoise_workspace_bytes", fn, workspace_bytes);
    const int64_t xb = ((B - 1) * x_stride + len_host) * 4;
    AREQUIRE(!(y && overlap(x, xb, y, ((B - 1) * y_stride + len_host) * 4)) && !(pcm && overlap(x, xb, pcm, ((B - 1) * pcm_stride + len_host) * 2)),
             "%s: an output overlaps the input (a tile reads its neighbours' samples)", fn);
    const int64_t tiles = (len_host + TILE - 1) / TILE;
    AREQUIRE(tiles < ((int64_t)1 << 31), "%s: %lld tiles per row", fn, (long long)tiles);
    const int G = batch_of(n_fft);
    hipLaunchKernelGGL(denoise_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(NT), lds_floats(n_fft, 1) * sizeof(float),
                       (hipStream_t)stream, x, (long)x_stride, (const long long*)len_dev, (long)len_host, bias_dev, strength, n_fft,
                       log2_of(n_fft / 2), hop, G, y, (long)y_stride, (short*)pcm, (long)pcm_stride);
    return launched(fn);
}

}  // extern "C"
