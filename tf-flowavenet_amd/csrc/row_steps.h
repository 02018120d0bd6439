// Per-row device steps of units that share nothing else: a length read from a device table and clamped where it is read
// (aux_kernels.hip, resample.hip, denoise.hip, melfront.hip, specdist.hip), and the 16-bit PCM sample of fwn_pcm16
// (aux_kernels.hip, denoise.hip).  Only those units include it (csrc/Makefile names it on their own lines).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// Every length comes from a table in device memory and is clamped to [0, T] where it is read, so no value of it loads or
// stores outside the buffer.
__device__ __forceinline__ long clamp_len(long len, long T) { return len < 0 ? 0 : (len > T ? T : len); }
// clip b's length: the device's own value (len_host without a table) clamped to [0, len_host], read here so that the host never
// sees it
__device__ __forceinline__ long clamp_len(const long long* len_dev, long b, long len_host) {
    return clamp_len(len_dev ? (long)len_dev[b] : len_host, len_host);
}

// int16 = rint((double)clamp(v, -1, 1) * 32767.0), NaN -> 0: synthesize.write_wav's float64 NumPy arithmetic bit for bit (the
// fp64 product of an fp32 value and 32767 is exact, so the one rounding is rint's half-to-even; the fp32 product would round
// twice at near-ties)
__device__ __forceinline__ short pcm16_of(float v) {
    v = (v != v) ? 0.0f : fminf(fmaxf(v, -1.0f), 1.0f);
    return (short)(int)rint((double)v * 32767.0);
}
