// Ragged mel front-end (include/fwn.h "ragged mel front-end"; DESIGN.md 6c has the definition): per clip the peak max|x|, the
// gain (x / peak) * rmax, the log-mel spectrogram of the normalised clip through the LDS FFT of stft_lds.h, and the reference's
// centre-padded audio - two launches for B clips of different lengths, no workspace.
//   peak_abs_kernel   a workgroup takes CHUNK consecutive samples of one clip, 16-byte loads where the address allows; |x| as a bit
//                     pattern is ordered like an unsigned integer (every NaN above +inf), so the maximum is an integer maximum:
//                     exact, whatever the order - in the lane, across the wave (shuffles), across the waves (LDS) and across the
//                     workgroups of a clip (one atomicMax each).  The output is cleared by a memset node in front of the launch.
//   mel_front_kernel  a workgroup owns FRAMES consecutive frames of one clip and transforms them G = batch_of(n_fft) at a time:
//     load     v_f[n] = w[n] xn[reflect(f hop + n - n_fft / 2)], xn = (x / peak) * rmax, as n_fft / 2 complex points
//     forward  the radix-2 Stockham passes, ping-pong between two LDS buffers
//     power    stft_lds.h's power_rows: |X[k]|^2, |X[nc - k]|^2 from Z[k], Z[nc - k] (split_pair) into LDS [G][nb], one lane per pair
//     mel      one lane per (frame, mel), stft_lds.h's mel_of: fmaf over the filter's bins [bands[m][0], bands[m][1]) in
//              ascending k, 20 log10, clip
//   and stores the hop-sample stretches of `audio` that belong to its frames.  Frames at or past the clip's own count, and every
//   frame of a clip that is silent, NaN or too short to reflect, are written as +0.  A frame is computed by the same
//   instructions whichever slot, workgroup, row or batch it lands in: its bits depend on the clip's samples in its support, on
//   N_b, peak[b], rmax and fb only.  The argument checks are audio_args.h's.
#include "audio_args.h"
#include "row_steps.h"
#include "stft_lds.h"

namespace {

using namespace stft_lds;
using namespace audio_args;

constexpr int FRAMES = 8;                   // frames a workgroup owns (fwn_mel_front_frames)
constexpr int CHUNK = 16384;                // samples of one clip a peak workgroup reads: 64 per lane

// |v| as bits: +0 for both zeros, 0x7f800000 for the infinities, anything above that for a NaN
__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }
__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }

__global__ __launch_bounds__(NT) void peak_abs_kernel(const float* __restrict__ x, long x_stride, const long long* __restrict__ len_dev,
                                                      long len_host, unsigned* __restrict__ peak_bits) {
    __shared__ unsigned part[NT / 64];
    const int tid = threadIdx.x;
    const long b = blockIdx.y;
    const long N = clamp_len(len_dev, b, len_host);
    const long s = (long)blockIdx.x * CHUNK;
    if (s >= N) return;                                        // nothing of the clip here (uniform: no barrier is skipped by part of a workgroup)
    const long n = N - s < CHUNK ? N - s : CHUNK;              // 1..CHUNK samples [s, s + n) of the clip
    const float* p = x + b * x_stride + s;
    long head = (long)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);        // scalars up to the first 16-byte boundary
    if (head > n) head = n;
    unsigned m = 0;
    if (tid < head) m = abs_bits(p[tid]);
    const float4* q = (const float4*)(p + head);
    const long nv = (n - head) >> 2;
    for (long i = tid; i < nv; i += NT) {
        const float4 v = q[i];
        m = umax(umax(m, abs_bits(v.x)), umax(abs_bits(v.y), umax(abs_bits(v.z), abs_bits(v.w))));
    }
    const long t0 = head + (nv << 2);                          // fewer than 4 left
    if (t0 + tid < n) m = umax(m, abs_bits(p[t0 + tid]));
    for (int d = 32; d >= 1; d >>= 1) m = umax(m, (unsigned)__shfl_xor((int)m, d, 64));
    if ((tid & 63) == 0) part[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NT / 64; ++w) m = umax(m, part[w]);
        if (m > 0x7f800000u) m = 0x7fc00000u;                  // one NaN for all of them
        if (m) atomicMax(peak_bits + b, m);
    }
}

template <bool GAIN>
__global__ __launch_bounds__(NT) void mel_front_kernel(const float* __restrict__ x, long x_stride, const long long* __restrict__ len_dev,
                                                       long len_host, const float* __restrict__ peak_dev, float rmax,
                                                       const float* __restrict__ fb, const int* __restrict__ bands, int n_fft, int lognc,
                                                       int hop, int n_mels, int G, float ref_db, float min_db, float* __restrict__ mel,
                                                       long mel_stride, float* __restrict__ audio, long audio_stride) {
    extern __shared__ float sm[];
    const int tid = threadIdx.x, h = n_fft / 2, nc = h, nb = h + 1;
    const long b = blockIdx.y;
    const long N = clamp_len(len_dev, b, len_host);
    const long F = 1 + N / hop, F_host = 1 + len_host / hop;
    const long f0 = (long)blockIdx.x * FRAMES;                 // < F_host by the grid
    const int rows = F_host - f0 < FRAMES ? (int)(F_host - f0) : FRAMES;       // the rows this workgroup writes
    const float peak = GAIN ? peak_dev[b] : 1.0f;
    const bool live = N >= h + 1 && (!GAIN || peak > 0.0f);    // not silent, not NaN, long enough to reflect
    const int nf = (!live || f0 >= F) ? 0 : (F - f0 < rows ? (int)(F - f0) : rows);    // the frames it computes
    const float* xrow = x + b * x_stride;
    float* mrow = mel + b * mel_stride + f0 * n_mels;
    for (int i = nf * n_mels + tid; i < rows * n_mels; i += NT) mrow[i] = 0.0f;
    if (audio) {                                               // samples [f0 hop, (f0 + rows) hop) of the padded clip
        float* arow = audio + b * audio_stride + f0 * hop;
        const long shift = f0 * hop - (F * hop - N) / 2;       // audio[i] = xn[i - pad_l]
        const int cnt = rows * hop;
        for (int s = tid; s < cnt; s += NT) {
            const long src = shift + s;
            float v = 0.0f;
            if (live && src >= 0 && src < N) {
                v = xrow[src];
                if (GAIN) v = (v / peak) * rmax;
            }
            arow[s] = v;
        }
    }
    if (nf == 0) return;

    Lds l = carve(sm, n_fft, G);
    float* pw = l.tail;                                        // [G][nb] power spectra
    fill_twiddles(l.tw, n_fft);
    __syncthreads();
    for (int g0 = 0; g0 < nf; g0 += G) {
        const int frames = nf - g0 < G ? nf - g0 : G;
        for (int g = 0; g < frames; ++g)
            load_frame<GAIN>(xrow, N, f0 + g0 + g, hop, n_fft, l.tw, (float*)(l.a + (size_t)g * nc), peak, rmax);
        __syncthreads();
        float2 *a = l.a, *bb = l.b;
        fft_passes(a, bb, l.tw, nc, lognc, frames, -1.0f);
        power_rows(a, l.tw, frames, nc, pw, nb);
        __syncthreads();
        for (int i = tid; i < frames * n_mels; i += NT) {      // lane owns (frame g, mel m)
            const int g = i / n_mels, m = i - g * n_mels;
            mrow[g0 * n_mels + i] = mel_of(fb, bands, m, nb, pw + (size_t)g * nb, ref_db, min_db);
        }
        __syncthreads();                                       // before the next batch is loaded over l.a and pw
    }
}

}  // namespace

extern "C" {

int fwn_mel_front_frames(int n_fft, int hop) {
    if (int rc = check_shape("fwn_mel_front_frames", n_fft, hop)) return rc;
    return FRAMES;
}

int fwn_clip_peak(const float* x, int64_t B, int64_t x_stride, const int64_t* len_dev, int64_t len_host, float* peak_out, void* stream) {
    const char* fn = "fwn_clip_peak";
    if (int rc = check_clips(fn, B, len_dev, len_host)) return rc;
    if (int rc = check_rows(fn, "x", x, 4, x_stride, len_host)) return rc;
    if (int rc = check_ptr(fn, "peak_out", peak_out, 4)) return rc;
    AREQUIRE(!overlap(x, ((B - 1) * x_stride + len_host) * 4, peak_out, B * 4), "%s: the output overlaps the input", fn);
    const int64_t chunks = (len_host + CHUNK - 1) / CHUNK;     // <= 2^26
    // +0: an empty clip's peak, and the maximum's start
    if (int rc = launched(fn, hipMemsetAsync(peak_out, 0, (size_t)B * 4, (hipStream_t)stream))) return rc;
    hipLaunchKernelGGL(peak_abs_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(NT), 0, (hipStream_t)stream, x, (long)x_stride,
                       (const long long*)len_dev, (long)len_host, (unsigned*)peak_out);
    return launched(fn);
}

int fwn_mel_front(const float* x, int64_t B, int64_t x_stride, const int64_t* len_dev, int64_t len_host, const float* peak_dev, float rmax,
                  const float* fb, const int32_t* bands, int n_fft, int hop, int n_mels, float ref_level_db, float min_level_db, float* mel,
                  int64_t mel_stride, float* audio, int64_t audio_stride, void* stream) {
    const char* fn = "fwn_mel_front";
    if (int rc = check_shape(fn, n_fft, hop)) return rc;
    if (int rc = check_clips(fn, B, len_dev, len_host)) return rc;
    if (int rc = check_rows(fn, "x", x, 4, x_stride, len_host)) return rc;
    if (int rc = check_ptr(fn, "peak_dev", peak_dev, 4, true)) return rc;
    if (int rc = check_ptr(fn, "fb", fb, 4)) return rc;
    if (int rc = check_ptr(fn, "bands", bands, 4, true)) return rc;
    AREQUIRE(n_mels >= 1 && n_mels <= 1024, "%s: n_mels %d outside 1..1024", fn, n_mels);
    AREQUIRE(min_level_db < 0.0f, "%s: min_level_db %g must be negative", fn, (double)min_level_db);
    AREQUIRE(rmax >= -3.0e38f && rmax <= 3.0e38f, "%s: rmax %g is infinite or NaN", fn, (double)rmax);
    AREQUIRE(!peak_dev || rmax > 0.0f, "%s: rmax %g must be positive when clips are normalised (peak_dev given)", fn, (double)rmax);
    const int64_t F_host = 1 + len_host / hop, mel_row = F_host * n_mels, audio_row = F_host * hop;
    if (int rc = check_rows(fn, "mel", mel, 4, mel_stride, mel_row)) return rc;
    if (audio) if (int rc = check_rows(fn, "audio", audio, 4, audio_stride, audio_row)) return rc;
    const int64_t groups = (F_host + FRAMES - 1) / FRAMES;
    AREQUIRE(groups < ((int64_t)1 << 31), "%s: %lld workgroups per row, past 2^31 - 1", fn, (long long)groups);
    const int64_t xb = ((B - 1) * x_stride + len_host) * 4;
    AREQUIRE(!overlap(x, xb, mel, ((B - 1) * mel_stride + mel_row) * 4) && !(audio && overlap(x, xb, audio, ((B - 1) * audio_stride + audio_row) * 4)),
             "%s: an output overlaps the input (a frame reads its neighbours' samples)", fn);
    const int G = batch_of(n_fft);
    const dim3 grid((unsigned)groups, (unsigned)B);
    const size_t lds = lds_floats(n_fft, G) * sizeof(float);
    if (peak_dev)
        hipLaunchKernelGGL(mel_front_kernel<true>, grid, dim3(NT), lds, (hipStream_t)stream, x, (long)x_stride, (const long long*)len_dev,
                           (long)len_host, peak_dev, rmax, fb, (const int*)bands, n_fft, log2_of(n_fft / 2), hop, n_mels, G, ref_level_db,
                           min_level_db, mel, (long)mel_stride, audio, (long)audio_stride);
    else
        hipLaunchKernelGGL(mel_front_kernel<false>, grid, dim3(NT), lds, (hipStream_t)stream, x, (long)x_stride, (const long long*)len_dev,
                           (long)len_host, peak_dev, rmax, fb, (const int*)bands, n_fft, log2_of(n_fft / 2), hop, n_mels, G, ref_level_db,
                           min_level_db, mel, (long)mel_stride, audio, (long)audio_stride);
    return launched(fn);
}

}  // extern "C"
