// The argument checks the audio units share (resample.hip, denoise.hip, melfront.hip, specdist.hip): host code only.  Every
// refusal is FWN_ERR_ARG through fwn_set_error, its message led by the entry point's name, and comes before any launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fwn.h"

int fwn_set_error(int code, const char* fmt, ...);      // api.hip: thread-local message of fwn_last_error()
#define AREQUIRE(cond, ...) do { if (!(cond)) return fwn_set_error(FWN_ERR_ARG, __VA_ARGS__); } while (0)

namespace audio_args {

constexpr int64_t MAX_LEN = (int64_t)1 << 40;
constexpr int64_t MAX_STRIDE = (int64_t)1 << 44;            // keeps B * stride * 4 inside int64

// the STFT's shape
inline int check_shape(const char* fn, int n_fft, int hop) {
    AREQUIRE(n_fft >= 32 && n_fft <= 4096 && (n_fft & (n_fft - 1)) == 0, "%s: n_fft %d is not a power of two in 32..4096", fn, n_fft);
    AREQUIRE(hop >= 1 && hop <= n_fft / 2, "%s: hop %d outside 1..n_fft/2 = %d", fn, hop, n_fft / 2);
    return FWN_OK;
}
// a device pointer to elements of elem_bytes (a power of two); NULL passes where the argument is optional
inline int check_ptr(const char* fn, const char* name, const void* p, int elem_bytes, bool optional = false) {
    AREQUIRE(p || optional, "%s: null pointer (%s)", fn, name);
    AREQUIRE((((uintptr_t)p) & (uintptr_t)(elem_bytes - 1)) == 0, "%s: a pointer is off its element's alignment (%s)", fn, name);
    return FWN_OK;
}
// B clips of min_len .. 2^40 samples, their own lengths in a device table or NULL
inline int check_clips(const char* fn, int64_t B, const int64_t* len_dev, int64_t len_host, int64_t min_len = 1) {
    if (int rc = check_ptr(fn, "len_dev", len_dev, 8, true)) return rc;
    AREQUIRE(B >= 1 && B < 65536, "%s: B %lld outside 1..65535", fn, (long long)B);
    AREQUIRE(len_host >= min_len && len_host <= MAX_LEN, "%s: clip length %lld outside %lld..2^40", fn, (long long)len_host, (long long)min_len);
    return FWN_OK;
}
// one array of rows, input or output: `row` elements of elem_bytes in use in each, `stride` elements apart
inline int check_rows(const char* fn, const char* name, const void* p, int elem_bytes, int64_t stride, int64_t row) {
    if (int rc = check_ptr(fn, name, p, elem_bytes)) return rc;
    AREQUIRE(stride >= row && stride <= MAX_STRIDE, "%s: row stride %lld of %s shorter than the row %lld, or above 2^44", fn,
             (long long)stride, name, (long long)row);
    return FWN_OK;
}
inline bool overlap(const void* p, int64_t pbytes, const void* q, int64_t qbytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)qbytes && b < a + (uintptr_t)pbytes;
}
// after a launch (or a memset): what the runtime made of it
inline int launched(const char* fn, hipError_t e = hipGetLastError()) {
    if (e != hipSuccess) return fwn_set_error(FWN_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
    return FWN_OK;
}

}  // namespace audio_args
