// The LDS short-time transform and the steps on its result that the STFT units share (denoise.hip, melfront.hip, specdist.hip):
//   carve, fill_twiddles, hann, load_frame, fft_passes, split_pair   all three: centred reflect-padded frames under the periodic
//       Hann window, taken as n_fft / 2 complex points z[m] = v[2m] + i v[2m + 1], radix-2 Stockham passes that ping-pong between
//       two LDS buffers, and the split that turns Z = FFT(z) into the bins of the real transform
//   power_rows, mel_of                                               melfront.hip and specdist.hip: |X[k]|^2 per slot, and one
//       mel of one power row (band clamp, filter sum, dB, clip) - one copy, so the two units' mels have the same bits
// Twiddles come from sincospif once per workgroup; the window is 0.5 - 0.5 cos from the same table.  Every function is a
// workgroup-wide step over NT lanes (mel_of: one lane's); a frame is computed by the same instructions whichever slot, workgroup
// or unit computes it (the locality rule).  A clip's length comes through row_steps.h's clamp_len.
//
// LDS banks: a pass reads src[j] and src[j + nc / 2] as 8-byte pairs at consecutive lanes (conflict-free) and writes dst at
// 2 (j - k) + k, k = j mod Ns: runs of Ns consecutive pairs, so the first passes (Ns = 1, 2) write at a 16-byte lane stride,
// two lanes of a 32-lane half per bank.  The autosort costs that instead of a bit-reversal pass.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace stft_lds {

constexpr int NT = 256;                     // lanes per workgroup

// frames transformed side by side: 2048 / n_fft, within 1..8 (two at n_fft 1024: every lane has two butterflies per pass)
inline int batch_of(int n_fft) { const int g = 2048 / n_fft; return g < 1 ? 1 : (g > 8 ? 8 : g); }
inline int log2_of(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
// floats of dynamic LDS: twiddles [n_fft / 2] pairs | two buffers [G][n_fft] | per_bin floats for each of n_fft / 2 + 2 bins
inline size_t lds_floats(int n_fft, int per_bin) { return (size_t)n_fft + 2 * (size_t)batch_of(n_fft) * n_fft + (size_t)per_bin * (n_fft / 2 + 2); }

struct Lds {
    float2* tw;        // [h]  (cos, sin)(2 pi j / n_fft)
    float2* a;         // [G][nc] complex: the loaded frames, and the result of an even number of passes
    float2* b;         // [G][nc]
    float* tail;       // what follows
};
__device__ __forceinline__ Lds carve(float* sm, int n_fft, int G) {
    Lds l;
    l.tw = (float2*)sm;
    l.a = (float2*)(sm + n_fft);
    l.b = l.a + (size_t)G * (n_fft / 2);
    l.tail = (float*)(l.b + (size_t)G * (n_fft / 2));
    return l;
}

__device__ __forceinline__ void fill_twiddles(float2* tw, int n_fft) {
    for (int j = threadIdx.x; j < n_fft / 2; j += NT) {
        float s, c;
        sincospif(2.0f * (float)j / (float)n_fft, &s, &c);
        tw[j] = make_float2(c, s);
    }
}
// periodic Hann w[n] = 0.5 - 0.5 cos(2 pi n / n_fft), the cosine of the second half being minus that of the first
__device__ __forceinline__ float hann(const float2* tw, int n, int h) {
    const float c = n < h ? tw[n].x : -tw[n - h].x;
    return 0.5f - 0.5f * c;
}

// frame f of a clip of N samples (N > n_fft / 2), windowed, into buf[n_fft].  GAIN: the sample is first normalised as
// (x / peak) * rmax - two separately rounded fp32 operations, the division IEEE.
template <bool GAIN = false>
__device__ __forceinline__ void load_frame(const float* __restrict__ xrow, long N, long f, int hop, int n_fft, const float2* tw,
                                           float* buf, float peak = 1.0f, float rmax = 1.0f) {
    const int h = n_fft / 2;
    const long j0 = f * hop - h;
    for (int n = threadIdx.x; n < n_fft; n += NT) {
        long j = j0 + n;
        if (j < 0) j = -j;                         // numpy 'reflect': the edge sample is not repeated
        if (j >= N) j = 2 * (N - 1) - j;
        if (GAIN) buf[n] = hann(tw, n, h) * ((xrow[j] / peak) * rmax);
        else buf[n] = hann(tw, n, h) * xrow[j];
    }
}

// log2(nc) radix-2 Stockham passes over `frames` slots of nc points each; sgn = -1 forward, +1 inverse (no scaling).  The result
// is in `a` again after an even number of passes and in `b` after an odd one: the pointers are swapped as the passes go.
__device__ __forceinline__ void fft_passes(float2*& a, float2*& b, const float2* tw, int nc, int lognc, int frames, float sgn) {
    const int half = nc >> 1;
    for (int p = 0; p < lognc; ++p) {
        const int Ns = 1 << p;
        for (int i = threadIdx.x; i < frames * half; i += NT) {
            const int g = i >> (lognc - 1), j = i & (half - 1), k = j & (Ns - 1);
            const float2* src = a + (size_t)g * nc;
            float2* dst = b + (size_t)g * nc;
            const float2 t = tw[k << (lognc - p)];             // e^(sgn 2 pi i k / (2 Ns))
            const float2 u = src[j], v = src[j + half];
            const float wr = t.x, wi = sgn * t.y;
            const float br = v.x * wr - v.y * wi, bi = v.x * wi + v.y * wr;
            const int j0 = ((j - k) << 1) + k;
            dst[j0] = make_float2(u.x + br, u.y + bi);
            dst[j0 + Ns] = make_float2(u.x - br, u.y - bi);
        }
        __syncthreads();
        float2* t = a; a = b; b = t;
    }
}

// bins k and nc - k (0 < k < nc / 2) of the real transform from Z = FFT(z): X[k] = Ze + T, X[nc - k] = conj(Ze - T) with
// Ze = (Z[k] + conj Z[nc - k]) / 2, Zo = (Z[k] - conj Z[nc - k]) / 2i, T = e^(-2 pi i k / n_fft) Zo
__device__ __forceinline__ void split_pair(float2 A, float2 B, float2 w, float2& Xk, float2& Xm) {
    const float zer = 0.5f * (A.x + B.x), zei = 0.5f * (A.y - B.y);
    const float zor = 0.5f * (A.y + B.y), zoi = -0.5f * (A.x - B.x);
    const float tr = w.x * zor + w.y * zoi, ti = w.x * zoi - w.y * zor;
    Xk = make_float2(zer + tr, zei + ti);
    Xm = make_float2(zer - tr, -(zei - ti));
}

// |X[k]|^2 of `frames` slots of Z = FFT(z) into rows pw + g * row, one lane per pair (k, nc - k), k = 0 .. nc / 2
__device__ __forceinline__ void power_rows(const float2* a, const float2* tw, int frames, int nc, float* pw, int row) {
    const int half = nc >> 1, per = half + 1;
    for (int i = threadIdx.x; i < frames * per; i += NT) {     // lane owns bins k and nc - k of slot g
        const int g = i / per, k = i - g * per;
        const float2* zf = a + (size_t)g * nc;
        float* pf = pw + (size_t)g * row;
        if (k == 0) {                                          // X[0] and X[nc] are real
            const float x0 = zf[0].x + zf[0].y, xn = zf[0].x - zf[0].y;
            pf[0] = x0 * x0;
            pf[nc] = xn * xn;
        } else if (k == half) {                                // its own partner: X = conj Z
            pf[half] = zf[half].x * zf[half].x + zf[half].y * zf[half].y;
        } else {
            float2 Xk, Xm;
            split_pair(zf[k], zf[nc - k], tw[k], Xk, Xm);
            pf[k] = Xk.x * Xk.x + Xk.y * Xk.y;
            pf[nc - k] = Xm.x * Xm.x + Xm.y * Xm.y;
        }
    }
}

// mel m of the power row pf[nb]: the filter fb[m][nb] summed by fmaf in ascending k over the bins [bands[m][0], bands[m][1])
// clamped to [0, nb) (all of them without `bands`), 20 log10 over the 1e-4 floor less ref_db, mapped from [min_db, 0] and
// clipped to [0, 1]
__device__ __forceinline__ float mel_of(const float* __restrict__ fb, const int* __restrict__ bands, int m, int nb, const float* pf,
                                        float ref_db, float min_db) {
    int lo = 0, hi = nb;
    if (bands) {
        lo = bands[2 * m] < 0 ? 0 : bands[2 * m];
        hi = bands[2 * m + 1] > nb ? nb : bands[2 * m + 1];
    }
    const float* w = fb + (long)m * nb;
    float acc = 0.0f;
    for (int k = lo; k < hi; ++k) acc = fmaf(w[k], pf[k], acc);
    const float db = 20.0f * log10f(fmaxf(1e-4f, acc)) - ref_db;
    return fminf(fmaxf((db - min_db) / (-min_db), 0.0f), 1.0f);
}

}  // namespace stft_lds
