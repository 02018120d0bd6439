// Band-limited rational sample-rate conversion (include/fwn.h "sample-rate conversion"; DESIGN.md has the definition).
//   up / down in lowest terms, q = max(up, down), Hh = zeros * q, K = 2 Hh / up + 1 taps per phase
//   y[m] = sum_k x[n0 - k] * T[r][k],   n0 = (m down + Hh) div up,   r = (m down + Hh) mod up,   x = 0 outside [0, N)
// fwn_resample_design builds T [up][K] on the host in fp64 (rounded once); resample_kernel is the one launch: a workgroup owns
// TILE consecutive outputs of one clip, stages the input span they read in LDS (converted to fp32, zeros outside the clip and
// outside the provided span - nothing out there is loaded) and each lane walks its phase row through L2.  A lane's sum is four
// fmaf chains over k = 0, 1, 2, 3 (mod 4), added as (a0 + a1) + (a2 + a3): the order is a function of k alone, so an output's
// bits do not depend on the tile, the row, in_start or m0.  A clip's length comes through row_steps.h's clamp_len; the argument
// checks the audio units share are audio_args.h's.
#include <math.h>

#include "audio_args.h"
#include "row_steps.h"

namespace {

using namespace audio_args;

constexpr int TILE = 256;                   // outputs per workgroup, one per lane
constexpr long LDS_FLOATS = 16384;          // 64 KiB of dynamic LDS: the largest staged span a launch may ask for
constexpr int64_t MAX_RATE = 1 << 20;       // up, down: keeps m * down and N * up inside int64 for N <= 2^40

int64_t gcd64(int64_t a, int64_t b) { while (b) { int64_t t = a % b; a = b; b = t; } return a; }
// floor / ceil of a / b for b > 0 and any sign of a
int64_t floordiv(int64_t a, int64_t b) { int64_t q = a / b; return (a % b != 0 && a < 0) ? q - 1 : q; }
int64_t ceildiv(int64_t a, int64_t b) { return -floordiv(-a, b); }

// I0 by its power series sum ((x / 2)^k / k!)^2: every term positive, so no cancellation; beta <= a few tens converges in < 100 terms
double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

__device__ __forceinline__ float load_sample(const float* x, long i) { return x[i]; }
__device__ __forceinline__ float load_sample(const short* x, long i) { return (float)x[i] * (1.0f / 32768.0f); }   // exact

template <typename XT>
__global__ __launch_bounds__(TILE) void resample_kernel(const XT* __restrict__ x, long x_stride, long in_start, long n_in,
                                                        const long long* __restrict__ len_dev, long len_host,
                                                        const float* __restrict__ T, int up, int down, long Hh, int K,
                                                        float* __restrict__ y, long y_stride, long m0, long n_req, int span_cap) {
    extern __shared__ float xs[];
    const int tid = threadIdx.x;
    const long b = blockIdx.y;
    const long N = clamp_len(len_dev, b, len_host);
    const long clip_out = (N * up + down - 1) / down;          // n_out(N)
    const long i0 = (long)blockIdx.x * TILE;                   // first requested output of this tile
    const long left = n_req - i0;
    const int cnt = left < TILE ? (int)left : TILE;
    const long mt = m0 + i0;
    float* yrow = y + b * y_stride + i0;
    if (mt >= clip_out) {                                      // the whole tile lies past the clip's last output
        if (tid < cnt) yrow[tid] = 0.0f;
        return;
    }
    const long mlast = (mt + cnt < clip_out ? mt + cnt : clip_out) - 1;
    const long base = (mt * down + Hh) / up - (K - 1);         // first staged clip sample (may be negative: zeros)
    long span = (mlast * down + Hh) / up - base + 1;
    if (span > span_cap) span = span_cap;                      // never true for the host's span_cap; keeps LDS writes inside it
    const XT* xrow = x + b * x_stride;
    for (long j = tid; j < span; j += TILE) {
        const long n = base + j, o = n - in_start;
        float v = 0.0f;
        if (n >= 0 && n < N && o >= 0 && o < n_in) v = load_sample(xrow, o);
        xs[j] = v;
    }
    __syncthreads();
    if (tid >= cnt) return;
    const long m = mt + tid;
    if (m >= clip_out) { yrow[tid] = 0.0f; return; }
    const long pos = m * down + Hh;
    const long n0 = pos / up;
    const float* t = T + (pos - n0 * up) * K;                  // phase row r = pos mod up
    int j0 = (int)(n0 - base);                                 // in [K - 1, span): xs[j0 - k] stays inside for k < K
    if (j0 > span_cap - 1) j0 = span_cap - 1;                  // as above: never true
    const float* xp = xs + j0;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    int k = 0;
    for (; k + 4 <= K; k += 4) {
        a0 = fmaf(xp[-k], t[k], a0);
        a1 = fmaf(xp[-k - 1], t[k + 1], a1);
        a2 = fmaf(xp[-k - 2], t[k + 2], a2);
        a3 = fmaf(xp[-k - 3], t[k + 3], a3);
    }
    if (k < K) a0 = fmaf(xp[-k], t[k], a0);
    if (k + 1 < K) a1 = fmaf(xp[-k - 1], t[k + 1], a1);
    if (k + 2 < K) a2 = fmaf(xp[-k - 2], t[k + 2], a2);
    yrow[tid] = (a0 + a1) + (a2 + a3);
}

int check_ratio(const char* fn, int up, int down, int zeros) {
    AREQUIRE(up >= 1 && down >= 1 && up <= MAX_RATE && down <= MAX_RATE, "%s: up %d / down %d outside 1..%d", fn, up, down, (int)MAX_RATE);
    AREQUIRE(gcd64(up, down) == 1, "%s: up %d / down %d is not in lowest terms (gcd %d)", fn, up, down, (int)gcd64(up, down));
    AREQUIRE(zeros >= 1 && zeros <= 64, "%s: zeros %d outside 1..64", fn, zeros);
    return FWN_OK;
}

}  // namespace

extern "C" {

int fwn_resample_taps(int up, int down, int zeros) {
    if (int rc = check_ratio("fwn_resample_taps", up, down, zeros)) return rc;
    const int64_t Hh = (int64_t)zeros * (up > down ? up : down);
    return (int)(2 * Hh / up + 1);
}

int fwn_resample_design(int up, int down, int zeros, double beta, double rolloff, float* table_host) {
    if (int rc = check_ratio("fwn_resample_design", up, down, zeros)) return rc;
    AREQUIRE(rolloff > 0.0 && rolloff <= 1.0, "fwn_resample_design: rolloff %g outside (0, 1]", rolloff);
    AREQUIRE(beta >= 0.0 && beta <= 100.0, "fwn_resample_design: beta %g outside [0, 100]", beta);   // (a NaN fails both)
    AREQUIRE(table_host, "fwn_resample_design: null table");
    const int64_t q = up > down ? up : down, Hh = (int64_t)zeros * q;
    const int64_t K = 2 * Hh / up + 1;
    const double i0b = bessel_i0(beta), gain = (double)up * rolloff / (double)q;
    for (int64_t r = 0; r < up; ++r)
        for (int64_t k = 0; k < K; ++k) {
            const int64_t j = r + k * up - Hh;
            double h = 0.0;
            if (j >= -Hh && j <= Hh) {
                const double t = rolloff * (double)j / (double)q, u = (double)j / (double)Hh;
                const double s = j == 0 ? 1.0 : sin(M_PI * t) / (M_PI * t);
                const double w2 = 1.0 - u * u;
                h = gain * s * bessel_i0(beta * sqrt(w2 > 0.0 ? w2 : 0.0)) / i0b;
            }
            table_host[r * K + k] = (float)h;
        }
    return FWN_OK;
}

int fwn_resample(const void* x, int x_pcm16, int64_t B, int64_t x_stride, int64_t in_start, int64_t n_in, const int64_t* len_dev,
                 int64_t len_host, const float* table_dev, int up, int down, int zeros, float* y, int64_t y_stride, int64_t m0,
                 int64_t n_out, void* stream) {
    if (int rc = check_ratio("fwn_resample", up, down, zeros)) return rc;
    AREQUIRE(x_pcm16 == 0 || x_pcm16 == 1, "fwn_resample: x_pcm16 must be 0 (float32) or 1 (16-bit PCM), got %d", x_pcm16);
    if (int rc = check_ptr("fwn_resample", "x", x, x_pcm16 ? 2 : 4)) return rc;
    if (int rc = check_ptr("fwn_resample", "table_dev", table_dev, 4)) return rc;
    if (int rc = check_ptr("fwn_resample", "y", y, 4)) return rc;
    if (int rc = check_clips("fwn_resample", B, len_dev, len_host, 0)) return rc;      // an empty clip is a clip
    AREQUIRE(in_start >= 0 && n_in >= 0 && in_start <= MAX_LEN && n_in <= MAX_LEN && m0 >= 0 && m0 <= MAX_LEN * MAX_RATE && n_out >= 1 &&
             n_out < ((int64_t)1 << 31) * TILE, "fwn_resample: bad span (in_start %lld, n_in %lld) or range (m0 %lld, n_out %lld)",
             (long long)in_start, (long long)n_in, (long long)m0, (long long)n_out);
    AREQUIRE(x_stride >= n_in && y_stride >= n_out, "fwn_resample: row strides %lld / %lld shorter than the rows %lld / %lld",
             (long long)x_stride, (long long)y_stride, (long long)n_in, (long long)n_out);
    const int64_t q = up > down ? up : down, Hh = (int64_t)zeros * q, K = 2 * Hh / up + 1;
    const int64_t span_cap = ((int64_t)(TILE - 1) * down) / up + K + 2;
    AREQUIRE(span_cap <= LDS_FLOATS, "fwn_resample: %d / %d with %d zeros stages %lld floats per tile, more than the %ld that fit",
             up, down, zeros, (long long)span_cap, LDS_FLOATS);
    // every requested output's support within [0, N) must lie in the provided span; N = len_host is the widest case (a device
    // length is clamped to it, and a shorter clip only drops samples from the top of a support)
    const int64_t clip_out = ceildiv(len_host * up, down);
    const int64_t mlast = (m0 + n_out < clip_out ? m0 + n_out : clip_out) - 1;
    if (mlast >= m0) {
        int64_t lo = ceildiv(m0 * down - Hh, up), hi = floordiv(mlast * down + Hh, up);
        if (lo < 0) lo = 0;
        if (hi > len_host - 1) hi = len_host - 1;
        AREQUIRE(lo > hi || (lo >= in_start && hi < in_start + n_in),
                 "fwn_resample: outputs [%lld, %lld] read clip samples [%lld, %lld], the provided span is [%lld, %lld)",
                 (long long)m0, (long long)mlast, (long long)lo, (long long)hi, (long long)in_start, (long long)(in_start + n_in));
    }
    const dim3 grid((unsigned)((n_out + TILE - 1) / TILE), (unsigned)B);
    const size_t lds = (size_t)span_cap * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    if (x_pcm16)
        hipLaunchKernelGGL(resample_kernel<short>, grid, dim3(TILE), lds, st, (const short*)x, (long)x_stride, (long)in_start, (long)n_in,
                           (const long long*)len_dev, (long)len_host, table_dev, up, down, (long)Hh, (int)K, y, (long)y_stride, (long)m0,
                           (long)n_out, (int)span_cap);
    else
        hipLaunchKernelGGL(resample_kernel<float>, grid, dim3(TILE), lds, st, (const float*)x, (long)x_stride, (long)in_start, (long)n_in,
                           (const long long*)len_dev, (long)len_host, table_dev, up, down, (long)Hh, (int)K, y, (long)y_stride, (long)m0,
                           (long)n_out, (int)span_cap);
    return launched("fwn_resample");
}

}  // extern "C"
