// HBM-bound helper kernels around the flow chain (gfx950):
//   weight-norm + bf16 packing (convolutional.py:73-80), mel upsampling by two transposed
//   convs (model.py:398-404), even/odd plane split/merge (the squeeze of model.py:226-239 is
//   pure index math on these planes), ActNorm data-dependent init (model.py:30-83) and the
//   prior / log-det finalisation (model.py:342-343).
#include "common.h"
#include "fwn_internal.h"
#include "row_steps.h"
#include "../../include/fwn.h"

// ---- weight-norm scale: scale[n] = g[n] / sqrt(max(sum_k V[k][n]^2, 1e-12)) ----------------
__global__ __launch_bounds__(1024) void wn_scale_kernel(const float* __restrict__ v, const float* __restrict__ g,
                                                        int k_src, int n_src, float* __restrict__ scale) {
    // 32 output channels x 32 K-partitions per workgroup (K is up to 10240 for the conditioning convs
    // and a training step recomputes every scale): coalesced over n, fixed-order tree over the partitions.
    __shared__ double red[32][33];
    const int nl = threadIdx.x & 31, kg = threadIdx.x >> 5;
    const int n = blockIdx.x * 32 + nl;
    double s = 0.0;
    if (n < n_src)
        for (int k = kg; k < k_src; k += 32) {
            const double x = v[(size_t)k * n_src + n];
            s += x * x;
        }
    red[kg][nl] = s;
    __syncthreads();
    for (int st = 16; st > 0; st >>= 1) {
        if (kg < st) red[kg][nl] += red[kg + st][nl];
        __syncthreads();
    }
    if (kg == 0 && n < n_src) scale[n] = (float)((double)g[n] / sqrt(fmax(red[0][nl], 1e-12)));
}

// ---- gather + scale + cast: out[n'][k'] = bf16(V[src_k[k']][src_n[n']] * scale[src_n[n']]) --
__global__ __launch_bounds__(256) void pack_kernel(const float* __restrict__ v, const float* __restrict__ scale,
                                                   const int* __restrict__ src_k, const int* __restrict__ src_n,
                                                   int n_src, int k_dst, long ld_dst, long total,
                                                   bf16* __restrict__ out) {
    // rows with src_n < 0 are skipped (left as the caller initialised them); columns with
    // src_k < 0 are written as zero (K padding).
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int kd = (int)(i % k_dst), nd = (int)(i / k_dst);
        const int sk = src_k[kd], sn = src_n[nd];
        if (sn < 0) continue;
        float val = 0.0f;
        if (sk >= 0) {
            val = v[(size_t)sk * n_src + sn];
            if (scale) val *= scale[sn];
        }
        out[(size_t)nd * ld_dst + kd] = (bf16)val;
    }
}

static inline int grid_for(long total);
// ---- e4m3 packing of the dilated conv weights (fp8 gate path, BASELINE configs[4]) ---------------------------------
// One power-of-two scale per packed matrix: e = floor(log2(448 / max|W|)), bytes = e4m3(W 2^e); the gate kernel undoes
// it with the MFMA's E8M0 scale operand.  absmax: max over all source elements of |v[k][n] scale[n] mul| (atomicMax on
// the bit pattern of a non-negative float: exact and order-independent); amax must be zeroed before the first call.
__global__ __launch_bounds__(256) void wn_absmax_kernel(const float* __restrict__ v, const float* __restrict__ scale,
                                                        int n_src, long total, float mul, unsigned int* __restrict__ amax) {
    float m = 0.0f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        float val = v[i] * mul;
        if (scale) val *= scale[i % n_src];
        m = fmaxf(m, fabsf(val));
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) m = fmaxf(m, __shfl_xor(m, s));
    if ((threadIdx.x & 63) == 0) atomicMax(amax, __float_as_uint(m));
}
__device__ __forceinline__ int e4m3_exponent(float amax) {      // e with amax 2^e <= 448 < amax 2^(e+1)
    if (!(amax > 0.0f)) return 0;
    int e = (int)floorf(log2f(448.0f / amax));
    while (ldexpf(amax, e) > 448.0f) --e;
    while (ldexpf(amax, e + 1) <= 448.0f) ++e;
    return e < -100 ? -100 : (e > 100 ? 100 : e);
}
__global__ __launch_bounds__(256) void pack_e4m3_kernel(const float* __restrict__ v, const float* __restrict__ scale,
                                                        const int* __restrict__ src_k, const int* __restrict__ src_n,
                                                        int n_src, int k_dst, long ld_dst, long total, float mul,
                                                        const float* __restrict__ amax, unsigned char* __restrict__ out,
                                                        int* __restrict__ exp_out) {
    const int e = e4m3_exponent(*amax);
    if (blockIdx.x == 0 && threadIdx.x == 0) *exp_out = e;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int kd = (int)(i % k_dst), nd = (int)(i / k_dst);
        const int sk = src_k[kd], sn = src_n[nd];
        if (sn < 0) continue;
        float val = 0.0f;
        if (sk >= 0) {
            val = v[(size_t)sk * n_src + sn] * mul;
            if (scale) val *= scale[sn];
        }
        out[(size_t)nd * ld_dst + kd] = (unsigned char)pack_e4m3x2(ldexpf(val, e), 0.0f);
    }
}
// bf16 [n] -> e4m3 [n] (tests, and callers that hold only the bf16 h)
__global__ __launch_bounds__(256) void cast_e4m3_kernel(const bf16* __restrict__ src, unsigned char* __restrict__ dst, long n) {
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 2; i < n; i += (long)gridDim.x * 512) {
        const float a = (float)src[i], b = i + 1 < n ? (float)src[i + 1] : 0.0f;
        const unsigned int pk = pack_e4m3x2(a, b);
        dst[i] = (unsigned char)pk;
        if (i + 1 < n) dst[i + 1] = (unsigned char)(pk >> 8);
    }
}
void fwn_launch_wn_absmax(const float* v, const float* scale, int k_src, int n_src, float mul, float* amax, hipStream_t st) {
    const long total = (long)k_src * n_src;
    hipLaunchKernelGGL(wn_absmax_kernel, dim3(grid_for(total)), dim3(256), 0, st, v, scale, n_src, total, mul, (unsigned int*)amax);
}
void fwn_launch_pack_e4m3(const float* v, const float* scale, const int* src_k, const int* src_n, int n_src, int k_dst,
                          int n_dst, long ld_dst, float mul, const float* amax, void* out, int* exp_out, hipStream_t st) {
    const long total = (long)k_dst * n_dst;
    hipLaunchKernelGGL(pack_e4m3_kernel, dim3(grid_for(total)), dim3(256), 0, st, v, scale, src_k, src_n, n_src, k_dst, ld_dst,
                       total, mul, amax, (unsigned char*)out, exp_out);
}
void fwn_launch_cast_e4m3(const void* src, void* dst, long n, hipStream_t st) {
    hipLaunchKernelGGL(cast_e4m3_kernel, dim3(grid_for((n + 1) / 2)), dim3(256), 0, st, (const bf16*)src, (unsigned char*)dst, n);
}

// ---- small parameter tables straight from the flat fp32 masters (training: refreshed every step, on the device) ------
// out[i] = F(post[i] * sum_t flat[idx[t][i]])  (idx < 0: term absent).  mode[i]: 0 = fp64 sum, identity; 1 = fp64 sum,
// exp (both rounded once, the host path's arithmetic); 2 / 3 = the same two in fp32, terms added in order - the
// arithmetic of the framework expressions these tables used to be computed with (bit-compatible with them).
__global__ __launch_bounds__(256) void gather_tables_kernel(const float* __restrict__ flat, const long long* __restrict__ idx,
                                                            int nterm, long total, const double* __restrict__ post,
                                                            const unsigned char* __restrict__ mode, float* __restrict__ out) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int md = mode[i];
        if (md < 2) {
            double acc = 0.0;
            for (int t = 0; t < nterm; ++t) {
                const long long ix = idx[(size_t)t * total + i];
                acc += ix >= 0 ? (double)flat[ix] : 0.0;
            }
            acc *= post[i];
            out[i] = (float)(md ? exp(acc) : acc);
        } else {
            float acc = 0.0f;
            bool first = true;
            for (int t = 0; t < nterm; ++t) {
                const long long ix = idx[(size_t)t * total + i];
                if (ix < 0) continue;
                acc = first ? flat[ix] : acc + flat[ix];
                first = false;
            }
            const float pf = (float)post[i];
            acc = md == 3 ? expf(pf * acc) : acc * pf;
            out[i] = acc;
        }
    }
}
// out[0] = sum_i in[i] (one workgroup, fixed order, fp64 accumulation)
__global__ __launch_bounds__(256) void sum_f32_kernel(const float* __restrict__ in, long n, float* __restrict__ out) {
    __shared__ double red[256];
    double a = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) a += (double)in[i];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)red[0];
}
// weight-normed up-sampling kernel (convolutional.py:179-186): out[k][kw] = v[k][kw] / sqrt(max(sum_k v[k][kw]^2, 1e-12)) * g
__global__ void upsample_wn_kernel(const float* __restrict__ v, const float* __restrict__ g, int s, float* __restrict__ out) {
    const int kw = threadIdx.x;
    if (kw >= 3) return;
    double ss = 0.0;
    for (int k = 0; k < 2 * s; ++k) ss += (double)v[k * 3 + kw] * (double)v[k * 3 + kw];
    const double nrm = sqrt(fmax(ss, 1e-12));
    for (int k = 0; k < 2 * s; ++k) out[k * 3 + kw] = (float)((double)v[k * 3 + kw] / nrm * (double)g[0]);
}
void fwn_launch_gather_tables(const float* flat, const long long* idx, int nterm, long total, const double* post,
                              const unsigned char* expflag, float* out, hipStream_t st) {
    hipLaunchKernelGGL(gather_tables_kernel, dim3(grid_for(total)), dim3(256), 0, st, flat, idx, nterm, total, post, expflag, out);
}
void fwn_launch_sum_f32(const float* in, long n, float* out, hipStream_t st) {
    hipLaunchKernelGGL(sum_f32_kernel, dim3(1), dim3(256), 0, st, in, n, out);
}
void fwn_launch_upsample_wn(const float* v, const float* g, int s, float* out, hipStream_t st) {
    hipLaunchKernelGGL(upsample_wn_kernel, dim3(1), dim3(64), 0, st, v, g, s, out);
}

// ---- grouped form of the two kernels above: a whole model's weight-norm scales and packed copies
// in two launches driven by device-resident job tables (a training step re-packs every weight from
// the fp32 masters; the tables are built once because master and output pointers are stable).
__global__ __launch_bounds__(1024) void wn_scale_jobs_kernel(const fwn_scale_job* __restrict__ jobs,
                                                             float* __restrict__ scales, int scale_ld) {
    __shared__ double red[32][33];
    const fwn_scale_job j = jobs[blockIdx.x];
    const int nl = threadIdx.x & 31, kg = threadIdx.x >> 5;
    const int n = blockIdx.y * 32 + nl;
    if (blockIdx.y * 32 >= j.n_src) return;
    double s = 0.0;
    if (n < j.n_src) {
        // 16 loads in flight per thread (a conditioning conv of the last block has 320 rows per thread: one dependent
        // load at a time was a 300 us latency chain); the squares are still added in ascending k
        typedef const __attribute__((address_space(1))) float* gf32;
        const gf32 v = (gf32)j.v + n;
        const size_t ld = (size_t)j.n_src;
        int k = kg;
        for (; k + 15 * 32 < j.k_src; k += 16 * 32) {
            float x[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) x[u] = v[(size_t)(k + 32 * u) * ld];
#pragma unroll
            for (int u = 0; u < 16; ++u) s += (double)x[u] * (double)x[u];
        }
        for (; k < j.k_src; k += 32) {
            const double x = v[(size_t)k * ld];
            s += x * x;
        }
    }
    red[kg][nl] = s;
    __syncthreads();
    for (int st = 16; st > 0; st >>= 1) {
        if (kg < st) red[kg][nl] += red[kg + st][nl];
        __syncthreads();
    }
    if (kg == 0 && n < j.n_src)
        scales[(size_t)blockIdx.x * scale_ld + n] = (float)((double)j.g[n] / sqrt(fmax(red[0][nl], 1e-12)));
}
// Every load is unconditional (indices clamped into range, the result selected afterwards): written as
// `valid ? v[..] : 0` each load sat in its own branch behind an s_waitcnt vmcnt(0) - one memory round trip per element.
template <bool HAS_SC>
__device__ __forceinline__ void pack_job_body(const fwn_pack_job& j, const float* __restrict__ sc, float (*tile)[65], int by, int ny) {
    bf16* out = (bf16*)j.out;
    const int kmax = j.k_dst - 1, nmax = j.n_dst - 1;
    // (scale * mul) first, like fwn_pack_bf16 fed a pre-multiplied scale: same bf16 bits
    // the job's pointers come from a table in memory: tell the compiler they are global (global_load, not flat_load)
    typedef const __attribute__((address_space(1))) float* gf32;
    typedef const __attribute__((address_space(1))) int* gi32;
    const gf32 jv = (gf32)j.v, scg = (gf32)sc;
    const gi32 jsk = (gi32)j.src_k, jsn = (gi32)j.src_n;
    auto value = [&](int kd, int nd, bool& skip) {
        const int sk = jsk[min(kd, kmax)], sn = jsn[min(nd, nmax)];
        skip = sn < 0 || nd > nmax;
        const int snc = max(sn, 0);
        const float v = jv[(size_t)max(sk, 0) * j.n_src + snc];
        const float m = HAS_SC ? scg[snc] * j.mul : j.mul;
        // a factor, not a select: a select on a loaded value is turned back into a branch around the load
        const float okf = (sk >= 0 && sn >= 0 && kd <= kmax && nd <= nmax) ? 1.0f : 0.0f;
        return v * m * okf;
    };
    if (j.transposed) {          // out[k][n], n contiguous like the source: straight through, 4 columns per thread
        const int n4 = (j.n_dst + 3) / 4;
        const long total = (long)j.k_dst * n4;
        const bool vec = (j.ld_dst & 3) == 0 && (((uintptr_t)out) & 7) == 0;
        // Fast form: the 4 columns map to 4 consecutive, 16-byte aligned source columns (identity / offset maps - every
        // training copy): one 16-byte load of the master and of the scales instead of 4 x (2 index loads + 2 loads).  The
        // per-element gathers of the general form made these jobs instruction-bound (2.1 TB/s against 3.3 for the
        // transposing jobs).  Same products in the same order: identical bits.
        const bool fast_ok = vec && (j.n_dst & 3) == 0 && (j.n_src & 3) == 0 && (((uintptr_t)j.v) & 15) == 0 && (((uintptr_t)j.src_n) & 15) == 0 &&
                             (!HAS_SC || (((uintptr_t)sc) & 15) == 0);
        typedef int vi4 __attribute__((ext_vector_type(4)));
        typedef float vf4 __attribute__((ext_vector_type(4)));
        typedef const __attribute__((address_space(1))) vi4* gi32x4;
        typedef const __attribute__((address_space(1))) vf4* gf32x4;
        for (long i = (long)by * 256 + threadIdx.x; i < total; i += (long)ny * 256) {
            const int kd = (int)(i / n4), nd0 = (int)(i % n4) * 4;
            if (fast_ok) {
                const vi4 sn = *(gi32x4)(jsn + nd0);
                const int sk = jsk[kd];
                if (sk >= 0 && sn.x >= 0 && (sn.x & 3) == 0 && sn.y == sn.x + 1 && sn.z == sn.x + 2 && sn.w == sn.x + 3) {
                    const vf4 v4 = *(gf32x4)(jv + (size_t)sk * j.n_src + sn.x);
                    vf4 m4 = {j.mul, j.mul, j.mul, j.mul};
                    if (HAS_SC) {
                        const vf4 s4 = *(gf32x4)(scg + sn.x);
                        m4 = vf4{s4.x * j.mul, s4.y * j.mul, s4.z * j.mul, s4.w * j.mul};
                    }
                    union { bf16 e[4]; uint2 u; } pk;
                    pk.e[0] = (bf16)(v4.x * m4.x * 1.0f); pk.e[1] = (bf16)(v4.y * m4.y * 1.0f);
                    pk.e[2] = (bf16)(v4.z * m4.z * 1.0f); pk.e[3] = (bf16)(v4.w * m4.w * 1.0f);
                    *(uint2*)(out + (size_t)kd * j.ld_dst + nd0) = pk.u;
                    continue;
                }
            }
            float v[4];
            bool skip[4], any_skip = false;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = value(kd, nd0 + e, skip[e]);
                any_skip = any_skip || skip[e];
            }
            bf16* o = out + (size_t)kd * j.ld_dst + nd0;
            if (vec && !any_skip) {
                union { bf16 e[4]; uint2 u; } pk;
#pragma unroll
                for (int e = 0; e < 4; ++e) pk.e[e] = (bf16)v[e];
                *(uint2*)o = pk.u;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (!skip[e]) o[e] = (bf16)v[e];
            }
        }
        return;
    }
    // out[n][k], k contiguous: a transpose of the source - 64 x 64 tiles through LDS so that both the fp32 reads
    // (n fastest) and the bf16 writes (k fastest) are coalesced
    const int tk = (j.k_dst + 63) / 64, tn = (j.n_dst + 63) / 64;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    for (int t = by; t < tk * tn; t += ny) {
        const int k0 = (t % tk) * 64, n0 = (t / tk) * 64;
        __syncthreads();
        float val[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {      // 16 independent gathers in flight
            bool skip;
            val[r] = value(k0 + ly + 4 * r, n0 + lx, skip);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) tile[ly + 4 * r][lx] = val[r];
        __syncthreads();
        // output rows whose source column is -1 belong to another job of the same matrix: left alone
        int sno[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) sno[r] = jsn[min(n0 + ly + 4 * r, nmax)];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int nd = n0 + ly + 4 * r, kd = k0 + lx;
            if (kd < j.k_dst && nd < j.n_dst && sno[r] >= 0) out[(size_t)nd * j.ld_dst + kd] = (bf16)tile[lx][ly + 4 * r];
        }
    }
}
__global__ __launch_bounds__(256) void pack_jobs_kernel(const fwn_pack_job* __restrict__ jobs,
                                                        const float* __restrict__ scales, int scale_ld) {
    __shared__ float tile[64][65];
    // blockIdx.y = job: the workgroups of a job are dispatched together and the jobs in table order - jobs that read the same
    // master (its inference packing and its transposed training copy: the host sorts the table by source) run back to back
    // and the second one finds the master in the Infinity Cache (with the job index in x every job was in flight at once)
    const fwn_pack_job j = jobs[blockIdx.y];
    if (j.scale_slot >= 0) pack_job_body<true>(j, scales + (size_t)j.scale_slot * scale_ld, tile, blockIdx.x, gridDim.x);
    else pack_job_body<false>(j, nullptr, tile, blockIdx.x, gridDim.x);
}
void fwn_launch_pack_jobs(const fwn_scale_job* sjobs, int nsjobs, const fwn_pack_job* jobs, int njobs, float* scales,
                          int scale_ld, hipStream_t st) {
    if (nsjobs > 0)
        hipLaunchKernelGGL(wn_scale_jobs_kernel, dim3(nsjobs, (scale_ld + 31) / 32), dim3(1024), 0, st, sjobs, scales, scale_ld);
    if (njobs > 0) hipLaunchKernelGGL(pack_jobs_kernel, dim3(160, njobs), dim3(256), 0, st, jobs, scales, scale_ld);
}

// ---- one Conv2DTranspose(filters=1, kernel (2s,3), strides (s,1), 'same') + LeakyReLU(0.4) --
// Gather form of SURVEY Appendix A: y[tau, w] = bias + sum over (i,k) with i*s + k - s/2 = tau
// and kw of x[i, w - kw + 1] * wk[k][kw].
__global__ __launch_bounds__(256) void upsample_kernel(const float* __restrict__ in, int B, int H, int W,
                                                       const float* __restrict__ wk, float bias_host,
                                                       const float* __restrict__ bias_dev, int s,
                                                       float* __restrict__ out_f32, bf16* __restrict__ out_planes) {
    const long total = (long)B * H * s * W;
    const int half = W >> 1;
    const float bias = bias_dev ? bias_dev[0] : bias_host;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int w = (int)(idx % W);
        const long rt = idx / W;
        const int tau = (int)(rt % ((long)H * s));
        const int b = (int)(rt / ((long)H * s));
        const int i1 = (tau + s / 2) / s;
        const int k1 = tau + s / 2 - i1 * s;
        // six taps, all loads unconditional (clamped addresses, validity as a factor): a branch per load costs a memory
        // round trip each.  The products are added in the same order as before.
        float xv[2][3], wv[2][3];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = i1 - j, k = k1 + j * s;
            const bool iok = i >= 0 && i < H;
            const float* xr = in + ((size_t)b * H + min(max(i, 0), H - 1)) * W;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int ws = w - kw + 1;
                const bool ok = iok && ws >= 0 && ws < W;
                xv[j][kw] = xr[min(max(ws, 0), W - 1)] * (ok ? 1.0f : 0.0f);
                wv[j][kw] = wk[min(k, 2 * s - 1) * 3 + kw];
            }
        }
        float acc = bias;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) acc += xv[j][kw] * wv[j][kw];
        acc = fmaxf(acc, 0.4f * acc);
        if (out_f32) out_f32[idx] = acc;
        if (out_planes) {
            // planes[q][b][tau][w - q*half], q = mel half (conditioning half of change_order)
            const int q = w >= half;
            out_planes[(((size_t)q * B + b) * ((size_t)H * s) + tau) * half + (w - q * half)] = (bf16)acc;
        }
    }
}

// The same stage, 8 consecutive mel bins per thread (W and W / 2 multiples of 8: the real 80-bin front-end): the two input
// rows arrive as 16-byte pieces, the output leaves as one 16-byte piece of bf16 (or two of fp32).  One element per thread
// was three integer divisions, twelve 4-byte loads and a 2-byte store per output: 50 us for the 10 M outputs of the bench
// batch's last stage.  The products are added in the order of upsample_kernel: bit-identical results.
__global__ __launch_bounds__(256) void upsample8_kernel(const float* __restrict__ in, int B, int H, int W,
                                                        const float* __restrict__ wk, float bias_host,
                                                        const float* __restrict__ bias_dev, int s,
                                                        float* __restrict__ out_f32, bf16* __restrict__ out_planes) {
    const int W8 = W >> 3, half = W >> 1;
    const long total = (long)B * H * s * W8;
    const float bias = bias_dev ? bias_dev[0] : bias_host;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int w = (int)(idx % W8) * 8;
        const long rt = idx / W8;
        const int tau = (int)(rt % ((long)H * s));
        const int b = (int)(rt / ((long)H * s));
        const int i1 = (tau + s / 2) / s;
        const int k1 = tau + s / 2 - i1 * s;
        float x[2][10], wv[2][3];        // x[j][e] = in[i_j][w - 1 + e], zero outside the row / the image
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = i1 - j, k = k1 + j * s;
            const float ok = (i >= 0 && i < H) ? 1.0f : 0.0f;
            const float* xr = in + ((size_t)b * H + min(max(i, 0), H - 1)) * W;
            const float4 a = *(const float4*)(xr + w), c = *(const float4*)(xr + w + 4);
            const float lo = xr[max(w - 1, 0)], hi = xr[min(w + 8, W - 1)];
            x[j][0] = lo * (w > 0 ? ok : 0.0f);
            x[j][1] = a.x * ok; x[j][2] = a.y * ok; x[j][3] = a.z * ok; x[j][4] = a.w * ok;
            x[j][5] = c.x * ok; x[j][6] = c.y * ok; x[j][7] = c.z * ok; x[j][8] = c.w * ok;
            x[j][9] = hi * (w + 8 < W ? ok : 0.0f);
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) wv[j][kw] = wk[min(k, 2 * s - 1) * 3 + kw];
        }
        float y[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float acc = bias;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) acc += x[j][e + 2 - kw] * wv[j][kw];      // in[i][w + e - kw + 1]
            y[e] = fmaxf(acc, 0.4f * acc);
        }
        if (out_f32) {
            float* o = out_f32 + (rt * W + w);
            *(float4*)o = make_float4(y[0], y[1], y[2], y[3]);
            *(float4*)(o + 4) = make_float4(y[4], y[5], y[6], y[7]);
        }
        if (out_planes) {
            const int q = w >= half;
            Pack16 pk;
#pragma unroll
            for (int e = 0; e < 8; ++e) pk.e[e] = (bf16)y[e];
            *(uint4*)(out_planes + (((size_t)q * B + b) * ((size_t)H * s) + tau) * half + (w - q * half)) = pk.u;
        }
    }
}

// ---- x[B][T] <-> planes[2][B][T/2] (even / odd samples) ------------------------------------
__global__ __launch_bounds__(256) void split_kernel(const float* __restrict__ x, long B, long T,
                                                    float* __restrict__ planes) {
    const long n = B * T, hT = T >> 1;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long b = i / T, t = i % T;
        planes[((t & 1) * B + b) * hT + (t >> 1)] = x[i];
    }
}
__global__ __launch_bounds__(256) void merge_kernel(const float* __restrict__ planes, long B, long T,
                                                    float* __restrict__ x) {
    const long n = B * T, hT = T >> 1;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long b = i / T, t = i % T;
        x[i] = planes[((t & 1) * B + b) * hT + (t >> 1)];
    }
}

// ---- per-clip row kernels: the pieces the ragged, synthesis, corpus and windowed kernels below share --------
// Grid: blockIdx.y = clip (row, slot, window), and the workgroups of blockIdx.x stride over that row alone - four 16-byte
// stores per thread if the whole row were written, at most about 2048 workgroups over all rows.
static inline long row_cap(long nrows) { return nrows < 2048 ? 2048 / nrows : 1; }
static inline dim3 row_grid(long bytes_per_row, long nrows) {
    const long want = (bytes_per_row + 16383) / 16384, cap = row_cap(nrows);
    return dim3((unsigned)(want < 1 ? 1 : (want > cap ? cap : want)), (unsigned)nrows);
}
// Every length and every core comes from a table in device memory and is clamped where it is read, so no value of it loads
// or stores outside the buffer: a length to [0, T] (row_steps.h's clamp_len); a core's offset to [0, L] and its count to what
// is left of L.
__device__ __forceinline__ void clamp_core(long& off, long& n, long L) {
    off = clamp_len(off, L);
    n = clamp_len(n, L - off);
}

// ---- ragged batches: the rows past each clip's own length, filled ------------------------------------
// buf [nclip][rows][row_bytes]; clip c keeps rows [0, len[c % nlen] / spr) and has every dword of the rest set to
// val(its byte offset from the clip's base).  The workgroups of a clip stride over its padded bytes only: a clip of full
// length costs each of them one load of len.  Whole 16-byte pieces between the first and the last 16-byte boundary of the
// padded range, single dwords (at most three each side) around them.
template <class Val>
__device__ __forceinline__ void fill_padded_rows(char* buf, long rows, size_t row_bytes, const int* __restrict__ len, int nlen,
                                                 int spr, Val val) {
    const long c = blockIdx.y;
    const long keep = clamp_len((long)len[c % nlen] / spr, rows);
    if (keep == rows) return;
    const uintptr_t clip = (uintptr_t)buf + (size_t)c * rows * row_bytes;
    const uintptr_t p0 = clip + (size_t)keep * row_bytes, p1 = clip + (size_t)rows * row_bytes;
    uintptr_t a0 = (p0 + 15) & ~(uintptr_t)15;
    if (a0 > p1) a0 = p1;
    uintptr_t a1 = p1 & ~(uintptr_t)15;
    if (a1 < a0) a1 = a0;
    auto at = [&](uintptr_t q) { return val(q - clip); };
    for (uintptr_t q = a0 + ((size_t)blockIdx.x * 256 + threadIdx.x) * 16; q < a1; q += (size_t)gridDim.x * 256 * 16)
        *(float4*)q = make_float4(at(q), at(q + 4), at(q + 8), at(q + 12));
    if (blockIdx.x == 0) {
        const uintptr_t h = p0 + (size_t)threadIdx.x * 4, t = a1 + (size_t)(threadIdx.x - 4) * 4;
        if (threadIdx.x < 4 && h < a0) *(float*)h = at(h);
        if (threadIdx.x >= 4 && threadIdx.x < 8 && t < p1) *(float*)t = at(t);
    }
}
// zero: what a clip on its own would find past its end
__global__ __launch_bounds__(256) void mask_rows_kernel(char* __restrict__ buf, long rows, long row_bytes,
                                                        const int* __restrict__ len, int nlen, int spr) {
    fill_padded_rows(buf, rows, (size_t)row_bytes, len, nlen, spr, [](size_t) { return 0.0f; });
}
// Ragged forward: the padded rows of a flow's x_a plane [nclip][rows][Ch] fp32 (Ch a power of two) hold -shift[tau].  The front
// conv applies ActNorm on the fly, (v + shift[tau]) * scale[tau]: a zero in a padded row would reach its +-1 taps as shift *
// scale, where a clip on its own is zero-padded AFTER ActNorm.  (-s + s) is exactly +0, so every product is an exact zero.
__global__ __launch_bounds__(256) void fill_neg_shift_kernel(float* __restrict__ buf, long rows, int Ch,
                                                             const float* __restrict__ shift, const int* __restrict__ len,
                                                             int nlen, int spr) {
    fill_padded_rows((char*)buf, rows, (size_t)Ch * 4, len, nlen, spr,
                     [=](size_t off) { return -shift[(off >> 2) & (size_t)(Ch - 1)]; });      // rows start at the clip's base
}

// ---- synthesis: the latent z drawn on the device ------------------------------------------------------------
// z [n][L] fp32 = temp * N(0,1) from Philox4x32-10 (include/fwn.h fwn_latent_normal has the stream's definition; the fp64
// restatement the tests compare against is tests/philox_ref.py).  Row r holds samples start[r] .. start[r] + L of clip
// clip_id[r]'s stream (start NULL: from sample 0, fwn_latent_normal's whole clips; a negative start is read as 0).  Sample i of
// a clip comes from counter (i / 4, 0, clip_id, 0), lane i % 4, alone, so it does not depend on n, on the clip's row, on L, on
// where the buffer starts or on how the stream is cut into windows.  The lanes of a row stride over the QUADS OF THE STREAM that
// overlap it (the first and the last may be partial when start or start + L is no multiple of 4); one lane runs one Philox
// call and stores its four samples as one 16-byte piece where that piece is wholly inside the row and 16-byte aligned, as
// single dwords otherwise.  Samples at j >= len[r] (clamped to [0, L]) are +0.  logf / sqrtf / sincospif are the library's
// accurate forms (the build has no fast-math): |z - fp64| stays within a few ulp of |z| <= 5.77 temp; 2 u2 is exact, so the
// sine and cosine see no argument rounding.
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}
__device__ __forceinline__ void box_muller(unsigned r, unsigned r2, float temp, float& a, float& b) {
    const float u1 = (float)((r >> 8) + 1u) * 0x1p-24f;          // (0, 1], exact
    const float u2x2 = (float)(r2 >> 8) * 0x1p-23f;              // 2 u2 in [0, 2), exact
    const float rad = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(u2x2, &s, &c);
    a = rad * c * temp;
    b = rad * s * temp;
}
__global__ __launch_bounds__(256) void latent_normal_at_kernel(float* __restrict__ z, long L, unsigned k0, unsigned k1,
                                                               const unsigned* __restrict__ clip_id,
                                                               const long long* __restrict__ start, float temp,
                                                               const int* __restrict__ len) {
    const long r = blockIdx.y;
    const long keep = len ? clamp_len(len[r], L) : L;
    const unsigned clip = clip_id ? clip_id[r] : (unsigned)r;
    long long s0 = start ? start[r] : 0;
    if (s0 < 0) s0 = 0;
    float* row = z + (size_t)r * L;
    const long long q0 = s0 >> 2, nq = ((s0 + L + 3) >> 2) - q0;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < nq; g += (long long)gridDim.x * 256) {
        const long long q = q0 + g;
        const long j0 = (long)(q * 4 - s0);                      // the quad's first sample, relative to the row: -3 .. L - 1
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (j0 < keep) {                                          // a quad wholly past the row's length draws nothing
            const uint4 w = philox4x32_10(make_uint4((unsigned)q, 0u, clip, 0u), k0, k1);
            box_muller(w.x, w.y, temp, v[0], v[1]);
            box_muller(w.z, w.w, temp, v[2], v[3]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j0 + e >= keep) v[e] = 0.0f;
        }
        float* p = row + j0;
        if (j0 >= 0 && j0 + 4 <= L && (((uintptr_t)p) & 15) == 0) {
            *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j0 + e >= 0 && j0 + e < L) p[e] = v[e];
        }
    }
}

// ---- training: a batch drawn from the device-resident corpus ---------------------------------------------------
// include/fwn.h fwn_corpus_draw has the layout and the stream's definition (tests/corpus_ref.py restates it).  blockIdx.y =
// slot b.  Every workgroup of a slot derives the slot's pick itself - one Philox call and two table reads, uniform over the
// workgroup - from the counter as it stands: nothing in this launch writes it (corpus_advance_kernel does, behind it in
// stream order).  The workgroups of a slot then stride over the row of x and the row of c (copy_row).  The first workgroup of
// a slot writes len and picks.  The table is the caller's: a negative frame count is read as 0, and no start leaves [0, n - F).
//
// copy_row: dst[0, keep) = src[0, keep), dst[keep, total) = +0, nothing of src from keep on loaded.  16-byte pieces where
// source, destination, keep and total are all 16-byte multiples - so a piece is either wholly copied or wholly zero - and
// dwords otherwise.  CUT = false: the caller's keep is total, and the tests against it are compiled out.
template <bool CUT>
__device__ __forceinline__ void copy_row(const float* src, float* dst, long keep, long total, long first, long stride) {
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0 && ((keep | total) & 3) == 0) {
        for (long q = first; q < (total >> 2); q += stride) {
            const long i = q * 4;
            *(float4*)(dst + i) = (!CUT || i < keep) ? *(const float4*)(src + i) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    } else {
        for (long i = first; i < total; i += stride) dst[i] = (!CUT || i < keep) ? src[i] : 0.0f;
    }
}
__global__ __launch_bounds__(256) void corpus_draw_kernel(const float* __restrict__ audio, const float* __restrict__ mel,
                                                          const long long* __restrict__ frame_off, unsigned long long n_utt, int hop,
                                                          int num_mels, int unit_frames, long F, unsigned k0, unsigned k1,
                                                          unsigned stream_id, const unsigned long long* counter,
                                                          float* __restrict__ x, float* __restrict__ c, int* __restrict__ len,
                                                          int* __restrict__ picks) {
    const unsigned b = blockIdx.y;
    const unsigned long long d = *counter;
    const uint4 r = philox4x32_10(make_uint4((unsigned)(d & 0xffffffffull), (unsigned)(d >> 32), b, stream_id), k0, k1);
    const long long u = (long long)(((unsigned long long)r.x * n_utt) >> 32);            // n_utt < 2^32: no overflow
    const long long f0 = frame_off[u];
    long long n = frame_off[u + 1] - f0;
    if (n < 0) n = 0;
    long long start = 0, frames;
    if (n > F) {
        start = (long long)__umul64hi((unsigned long long)r.y << 32, (unsigned long long)(n - F));      // (r1 (n - F)) >> 32
        frames = F;
    } else {
        frames = n / unit_frames * unit_frames;
    }
    const long long row0 = f0 + start;
    const long first = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    copy_row<true>(audio + row0 * hop, x + (long long)b * F * hop, (long)(frames * hop), F * hop, first, stride);
    copy_row<true>(mel + row0 * num_mels, c + (long long)b * F * num_mels, (long)(frames * num_mels), F * num_mels, first, stride);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        len[b] = (int)(frames * hop);
        if (picks) {
            picks[2 * b] = (int)u;
            picks[2 * b + 1] = (int)start;
        }
    }
}
// one lane, behind the gather in stream order: the draw counter moves on (a plain load and a plain vector store)
__global__ void corpus_advance_kernel(unsigned long long* counter) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *counter = *counter + 1ull;
}

// ---- synthesis: fp32 waveform -> 16-bit PCM ------------------------------------------------------------------
// x [B][T] fp32 -> pcm [B][T] int16 = pcm16_of(x) (row_steps.h: synthesize.write_wav's float64 NumPy arithmetic bit for bit).
// Samples at i >= len[b] (clamped) are 0.
// One row: pr[0, n) = pcm16_of(xr[i]) for i < keep, 0 from keep on - and nothing of xr from keep on is loaded.  Between the
// first and the last 16-byte boundary of pr, one lane turns eight samples (two 16-byte loads) into one 16-byte store - where
// xr is 16-byte aligned at that first boundary too; the up to seven samples on either side go one by one, and so does the
// whole row where xr and pr disagree about their 16-byte phase.  CUT = false: the caller's keep is n, and the tests against it
// are compiled out (left in, the launch over a group's 8 cores of 262 144 samples took 5.3 us against 3.5 - 4.0).
template <bool CUT>
__device__ __forceinline__ void pcm16_row(const float* __restrict__ xr, short* __restrict__ pr, long n, long keep, long first,
                                          long stride) {
    // [a0, a1): the samples of the row whose pcm bytes form whole aligned 16-byte pieces
    long a0 = (long)(((16 - (((uintptr_t)pr) & 15)) & 15) >> 1);
    if (a0 > n) a0 = n;
    long a1 = a0 + ((n - a0) & ~7L);
    if ((((uintptr_t)(xr + a0)) & 15) != 0) a1 = a0 = 0;         // phases disagree: everything goes through the side loop
    for (long g = first; g < ((a1 - a0) >> 3); g += stride) {
        const long i0 = a0 + g * 8;
        union { short s[8]; uint4 u; } o;
        if (CUT && i0 >= keep) {
            o.u = make_uint4(0u, 0u, 0u, 0u);                     // past the clip's end: nothing is loaded
        } else {
            const float4 lo = *(const float4*)(xr + i0), hi = *(const float4*)(xr + i0 + 4);
            const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) o.s[e] = (!CUT || i0 + e < keep) ? pcm16_of(v[e]) : (short)0;
        }
        *(uint4*)(pr + i0) = o.u;
    }
    const long nside = a0 + (n - a1);                             // head [0, a0) and tail [a1, n)
    for (long j = first; j < nside; j += stride) {
        const long i = j < a0 ? j : a1 + (j - a0);
        pr[i] = (!CUT || i < keep) ? pcm16_of(xr[i]) : (short)0;
    }
}
__global__ __launch_bounds__(256) void pcm16_kernel(const float* __restrict__ x, short* __restrict__ pcm, long T,
                                                    const int* __restrict__ len) {
    const long b = blockIdx.y;
    pcm16_row<true>(x + (size_t)b * T, pcm + (size_t)b * T, T, len ? clamp_len(len[b], T) : T, (long)blockIdx.x * 256 + threadIdx.x,
                    (long)gridDim.x * 256);
}

// ---- windowed synthesis: the mel rows of a window, the cores of a group (include/fwn.h) ----------
// dst [n][count] fp32: row r = the count floats of src from float offset src_row[r] * row_floats (64-bit: the source is a flat
// buffer of whole clips, or of many), through copy_row.  A negative offset is read as 0.
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ src, const long long* __restrict__ src_row,
                                                            long row_floats, float* __restrict__ dst, long count) {
    const long r = blockIdx.y;
    long long s0 = src_row[r];
    if (s0 < 0) s0 = 0;
    copy_row<false>(src + (size_t)s0 * (size_t)row_floats, dst + (size_t)r * count, count, count,
                    (long)blockIdx.x * 256 + threadIdx.x, (long)gridDim.x * 256);
}

// The cores of a group: for row r of x [n][L] fp32, the core_len[r] samples from core_off[r] (clamped into the row) go to
// pcm + out_off[r] as 16-bit PCM (pcm16_row on the core) and / or to wav + out_off[r] as they are; out_off is the caller's
// (64-bit).  Nothing outside [out_off, out_off + core_len) is written.  The waveform is not copy_row's rule: its destination
// starts anywhere, so it goes in 16-byte pieces between the DESTINATION's boundaries where the source agrees, dwords otherwise.
__global__ __launch_bounds__(256) void window_scatter_kernel(const float* __restrict__ x, long L, const int* __restrict__ core_off,
                                                             const int* __restrict__ core_len,
                                                             const long long* __restrict__ out_off, short* __restrict__ pcm,
                                                             float* __restrict__ wav) {
    const long r = blockIdx.y;
    long off = core_off[r], n = core_len[r];
    clamp_core(off, n, L);
    const float* xr = x + (size_t)r * L + off;
    const long long o0 = out_off[r];
    const long first = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    if (pcm) pcm16_row<false>(xr, pcm + o0, n, n, first, stride);
    if (wav) {
        float* wr = wav + o0;
        long a0 = (long)(((16 - (((uintptr_t)wr) & 15)) & 15) >> 2);
        if (a0 > n) a0 = n;
        long a1 = a0 + ((n - a0) & ~3L);
        if ((((uintptr_t)(xr + a0)) & 15) != 0) a1 = a0 = 0;
        for (long g = first; g < ((a1 - a0) >> 2); g += stride) *(float4*)(wr + a0 + g * 4) = *(const float4*)(xr + a0 + g * 4);
        const long nside = a0 + (n - a1);
        for (long j = first; j < nside; j += stride) {
            const long i = j < a0 ? j : a1 + (j - a0);
            wr[i] = xr[i];
        }
    }
}

// ---- ragged and windowed forward: one flow's log-det terms per clip, over a range of its rows ------------
// Z [nclip][rows][2 Ch] fp32 is what the saving tail keeps of the ZeroConv (fwn_tail_chain.save_z): log_s = Z[row][tau] *
// ez[(tau / 32) * 64 + tau % 32] for tau < Ch (the pair-tile order of fwn_flow_desc.ezero).  Clip c's range is rows
// [off[c] / spr, off[c] / spr + cnt[c % ncnt] / spr) - off NULL: from row 0, the ragged pass's [0, len / spr) - the start
// clamped to [0, rows], the count to what is left.  blockIdx.y = clip, blockIdx.x = chunk: the workgroups of a clip stride
// over its range only - no row outside it is loaded - and each leaves the fp64 sum of -log_s over its share in
// acc[clip][chunk] (a workgroup without a share leaves 0).  The order of every sum is fixed by the grid: no atomics.
// 16-byte loads where the range's first row is 16-byte aligned: Ch / 4 per row from Ch = 4 on, one per row at Ch = 2.  At
// Ch = 1 (two rows per 16 bytes, a row is 8 bytes) a range whose first row sits 8 bytes off peels that row as a dword and goes
// on in 16-byte loads - the peeled form, not single dwords throughout - and one that then ends on an odd row takes its last
// as a dword.  A whole-model pass never peels without a start table: a clip there has an even number of rows at Ch = 1 (block
// 0), so every clip's base is 16-byte aligned; only fwn_ragged_logdet_rows with an odd row count per clip reaches the peel
// from row 0.  Single dwords everywhere else.  an (may be NULL): chunk 0 also leaves the flow's ActNorm term sum_tau 3 logs_a
// + 3 logs_b in acc[clip][nslot - 1].
__device__ __forceinline__ float ez_of(const float* __restrict__ ez, int tau) { return ez[(tau >> 5) * 64 + (tau & 31)]; }
__global__ __launch_bounds__(256) void range_logdet_kernel(const float* __restrict__ Z, long rows, int Ch,
                                                           const float* __restrict__ ez, const float* __restrict__ an,
                                                           const int* __restrict__ off, const int* __restrict__ cnt, int ncnt,
                                                           int spr, double* __restrict__ acc, int nslot) {
    __shared__ double red[256];
    const long c = blockIdx.y;
    long r0 = off ? (long)off[c] / spr : 0, keep = (long)cnt[c % ncnt] / spr;
    clamp_core(r0, keep, rows);
    const float* zc = Z + ((size_t)c * rows + (size_t)r0) * 2 * Ch;
    const long stride = (long)gridDim.x * 256, first = (long)blockIdx.x * 256 + threadIdx.x;
    double s = 0.0;
    if (Ch >= 4 && ((uintptr_t)zc & 15) == 0) {
        const int upr = Ch >> 2;                              // 16-byte pieces of log_s per row
        const long n = keep * upr;
        for (long i = first; i < n; i += stride) {
            const long row = i / upr;
            const int t0 = (int)(i - row * upr) * 4;
            const float4 v = *(const float4*)(zc + (size_t)row * 2 * Ch + t0);
            const float* e = ez + (t0 >> 5) * 64 + (t0 & 31);                         // four channels of one pair tile
            s -= (double)v.x * (double)e[0] + (double)v.y * (double)e[1] + (double)v.z * (double)e[2] + (double)v.w * (double)e[3];
        }
    } else if (Ch == 2 && ((uintptr_t)zc & 15) == 0) {
        const double e0 = ez[0], e1 = ez[1];
        for (long i = first; i < keep; i += stride) {
            const float4 v = *(const float4*)(zc + (size_t)i * 4);                    // log_s 0, log_s 1, t 0, t 1
            s -= (double)v.x * e0 + (double)v.y * e1;
        }
    } else if (Ch == 1 && ((uintptr_t)zc & 7) == 0) {
        const double e0 = ez[0];
        const long head = (((uintptr_t)zc & 15) != 0 && keep > 0) ? 1 : 0;            // an odd first row
        const float* zp = zc + head * 2;
        const long left = keep - head;
        for (long i = first; i < (left >> 1); i += stride) {
            const float4 v = *(const float4*)(zp + (size_t)i * 4);                    // two rows of (log_s, t)
            s -= (double)v.x * e0 + (double)v.z * e0;
        }
        if (first == 0) {
            if (head) s -= (double)zc[0] * e0;
            if (left & 1) s -= (double)zp[(size_t)(left - 1) * 2] * e0;
        }
    } else {
        const long n = keep * Ch;
        for (long i = first; i < n; i += stride) {
            const long row = i / Ch;
            const int tau = (int)(i - row * Ch);
            s -= (double)zc[(size_t)row * 2 * Ch + tau] * (double)ez_of(ez, tau);
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    double* out = acc + (size_t)c * nslot;
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
    if (an && blockIdx.x == 0) {
        double a = 0.0;
        for (int tau = threadIdx.x; tau < Ch; tau += 256) a += (double)an[3 * Ch + tau] + (double)an[7 * Ch + tau];
        __syncthreads();
        red[threadIdx.x] = a;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if (threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[nslot - 1] = red[0];
    }
}

// ---- ragged forward: out[0][b] = log_p, out[1][b] = logdet of clip b ------------------------------------
// One workgroup per clip.  acc [nflows][nclip][nslot] fp64: what range_logdet_kernel left for every flow, flow f of block
// f / n_flow with Ch = 2^(f / n_flow) channels per plane.  A flow's term is mean_C(3 logs) + mean(-log_s) / 2 over the clip's
// own rows (model.py:80,135): sum_an / (2 Ch) + sum(-log_s) / (2 rows Ch), and 2 rows Ch = len at every block.  The prior is
// the mean of 0.5 (-log 2 pi - z^2) over [0, len / 2) of both planes (model.py:342-343): nothing past a clip's end is
// loaded.  Everything is added in fp64 in an order the launch fixes.
__global__ __launch_bounds__(256) void ragged_finish_kernel(const float* __restrict__ planes, long nclip, long T,
                                                            const double* __restrict__ acc, int nflows, int n_flow, int nslot,
                                                            const int* __restrict__ len, float* __restrict__ out) {
    __shared__ double r1[256], r2[256];
    const long c = blockIdx.x, hT = T >> 1;
    const long n = clamp_len(len[c], T), hn = n >> 1;
    double s = 0.0, ld = 0.0;
    for (int q = 0; q < 2; ++q) {
        const float* z = planes + ((size_t)q * nclip + c) * hT;
        long i = 0;
        if (((uintptr_t)z & 15) == 0) {
            for (long k = threadIdx.x; k < (hn >> 2); k += 256) {
                const float4 v = *(const float4*)(z + k * 4);
                s += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
            }
            i = hn & ~3L;
        }
        for (long k = i + threadIdx.x; k < hn; k += 256) s += (double)z[k] * z[k];
    }
    for (int f = 0; f < nflows; ++f) {
        const double* a = acc + ((size_t)f * nclip + c) * nslot;
        double raw = 0.0;
        for (int k = threadIdx.x; k < nslot - 1; k += 256) raw += a[k];
        ld += raw / (double)(n > 0 ? n : 1);
        if (threadIdx.x == 0) ld += a[nslot - 1] / (double)(2 << (f / n_flow));
    }
    r1[threadIdx.x] = s;
    r2[threadIdx.x] = ld;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) { r1[threadIdx.x] += r1[threadIdx.x + st]; r2[threadIdx.x] += r2[threadIdx.x + st]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[c] = (float)(0.5 * (-1.8378770664093453 - r1[0] / (double)(n > 0 ? n : 1)));
        out[nclip + c] = (float)r2[0];
    }
}

// ---- windowed forward: the sums and the latent of a group's cores (include/fwn.h) --------------------------
// One workgroup per window c of a group: its four partial sums -> out[slot[c]][0 .. 4) fp64 (a negative slot writes nothing):
//   [0] sum of z^2 over the core's elements [off / 2, (off + len) / 2) of both final planes [2][n][L / 2] (off = core_off[c]
//       clamped to [0, L], len = core_len[c] to [0, L - off]; nothing outside is loaded),
//   [1] sum over the flows, in flow order, of their chunk sums of -log_s (acc [nflows][n][nslot], range_logdet_kernel's),
//   [2] sum over the flows of their ActNorm terms, sum_tau(3 logs) / (2 Ch) - the same for every window,
//   [3] len, the number of samples these sums cover.
// fp64 throughout, in an order the launch fixes: no atomics.
__global__ __launch_bounds__(256) void window_sums_kernel(const float* __restrict__ planes, long n, long L,
                                                          const int* __restrict__ core_off, const int* __restrict__ core_len,
                                                          const double* __restrict__ acc, int nflows, int n_flow, int nslot,
                                                          const int* __restrict__ slot, double* __restrict__ out) {
    __shared__ double r1[256], r2[256];
    const long c = blockIdx.x, hL = L >> 1;
    long off = core_off[c], len = core_len[c];
    clamp_core(off, len, L);
    const long e0 = off >> 1, e1 = (off + len) >> 1;
    double s = 0.0, ld = 0.0, an = 0.0;
    for (int q = 0; q < 2; ++q) {
        const float* z = planes + ((size_t)q * n + c) * hL;
        long a0 = e0 + (long)(((16 - ((uintptr_t)(z + e0) & 15)) & 15) >> 2);         // the first 16-byte boundary inside the core
        if (a0 > e1) a0 = e1;
        const long a1 = a0 + ((e1 - a0) & ~3L);
        for (long k = threadIdx.x; k < ((a1 - a0) >> 2); k += 256) {
            const float4 v = *(const float4*)(z + a0 + k * 4);
            s += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
        }
        const long nside = (a0 - e0) + (e1 - a1);                                      // head [e0, a0) and tail [a1, e1)
        for (long j = threadIdx.x; j < nside; j += 256) {
            const long i = j < a0 - e0 ? e0 + j : a1 + (j - (a0 - e0));
            s += (double)z[i] * z[i];
        }
    }
    for (int f = 0; f < nflows; ++f) {
        const double* a = acc + ((size_t)f * n + c) * nslot;
        for (int k = threadIdx.x; k < nslot - 1; k += 256) ld += a[k];
        if (threadIdx.x == 0) an += a[nslot - 1] / (double)(2 << (f / n_flow));
    }
    r1[threadIdx.x] = s;
    r2[threadIdx.x] = ld;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) { r1[threadIdx.x] += r1[threadIdx.x + st]; r2[threadIdx.x] += r2[threadIdx.x + st]; }
        __syncthreads();
    }
    if (threadIdx.x == 0 && slot[c] >= 0) {
        double* o = out + (size_t)slot[c] * 4;
        o[0] = r1[0]; o[1] = r2[0]; o[2] = an; o[3] = (double)len;
    }
}

// The cores of a group's latent in TIME order: sample s of window c lives in plane (s & 1) ^ swapped at element s / 2 (the
// planes hold the even and the odd samples; every flow exchanges them, so after an odd number of flows they are swapped -
// z_planes_to_squeezed followed by n_block un-squeezes is exactly this), and z[out_off[c] + i] = sample core_off[c] + i for
// i < core_len[c], the core clamped into the window as above.  A lane takes a pair of samples - one element of either
// plane, one 8-byte store where the core starts on an even sample and the destination is 8-byte aligned, single samples
// otherwise.  Nothing outside [out_off, out_off + core_len) is written.
__global__ __launch_bounds__(256) void window_latent_kernel(const float* __restrict__ planes, long n, long L, int swapped,
                                                            const int* __restrict__ core_off, const int* __restrict__ core_len,
                                                            const long long* __restrict__ out_off, float* __restrict__ z) {
    const long c = blockIdx.y, hL = L >> 1;
    long off = core_off[c], len = core_len[c];
    clamp_core(off, len, L);
    const float* even = planes + ((size_t)(swapped ? 1 : 0) * n + c) * hL;             // where the even samples are
    const float* odd = planes + ((size_t)(swapped ? 0 : 1) * n + c) * hL;
    float* zr = z + out_off[c];
    const long first = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    if ((off & 1) == 0 && ((uintptr_t)zr & 7) == 0) {
        const long e0 = off >> 1;
        for (long k = first; k < (len >> 1); k += stride) *(float2*)(zr + 2 * k) = make_float2(even[e0 + k], odd[e0 + k]);
        if ((len & 1) && first == 0) zr[len - 1] = even[e0 + (len >> 1)];
    } else {
        for (long i = first; i < len; i += stride) {
            const long sidx = off + i;
            zr[i] = ((sidx & 1) ? odd : even)[sidx >> 1];
        }
    }
}

// Per clip c: the partial sums of its windows, slots [slot0[c], slot0[c] + nwin[c]) of part [.][4] (window_sums_kernel), added
// in window order by one lane - so the result depends on neither the grouping nor the order the groups ran in - and
// out[0][c] = log_p = 0.5 (-log 2 pi - sum z^2 / t), out[1][c] = logdet = ActNorm term (the first window's) + sum(-log_s) / t,
// t = the samples the windows cover.  fwn_model_forward_ragged's layout of out2B.
__global__ __launch_bounds__(64) void windows_finish_kernel(const double* __restrict__ part, const int* __restrict__ slot0,
                                                            const int* __restrict__ nwin, long nclip, float* __restrict__ out) {
    const long c = (long)blockIdx.x * 64 + threadIdx.x;
    if (c >= nclip) return;
    const long s0 = slot0[c] < 0 ? 0 : slot0[c], nw = nwin[c] < 0 ? 0 : nwin[c];
    double z2 = 0.0, ls = 0.0, t = 0.0;
    for (long k = 0; k < nw; ++k) {
        const double* p = part + (size_t)(s0 + k) * 4;
        z2 += p[0]; ls += p[1]; t += p[3];
    }
    const double an = nw > 0 ? part[(size_t)s0 * 4 + 2] : 0.0, inv = 1.0 / (t > 0.0 ? t : 1.0);
    out[c] = (float)(0.5 * (-1.8378770664093453 - z2 * inv));
    out[nclip + c] = (float)(an + ls * inv);
}

// ---- ActNorm data-dependent init for one flow -----------------------------------------------
// One workgroup per (plane role, channel). an[role][0..3][tau] = shift b, scale exp(3 logs),
// inverse scale, 3*logs.  model.py:55-56 (b = -mean), :65-71 (logs from mean((x+b)^2)).
__device__ double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}
__global__ __launch_bounds__(256) void ddi_kernel(const float* __restrict__ xa, const float* __restrict__ xb,
                                                  int M, int Ch, float* __restrict__ an) {
    __shared__ double red[256];
    const int role = blockIdx.x / Ch, tau = blockIdx.x % Ch;
    const float* src = role ? xb : xa;
    double s = 0.0;
    for (int r = threadIdx.x; r < M; r += 256) s += src[(size_t)r * Ch + tau];
    const double mean = block_sum(s, red) / M;
    const float bshift = (float)(-mean);
    double s2 = 0.0;
    for (int r = threadIdx.x; r < M; r += 256) {
        const double d = (double)(src[(size_t)r * Ch + tau] + bshift);
        s2 += d * d;
    }
    const double var = block_sum(s2, red) / M;
    if (threadIdx.x == 0) {
        const double den = sqrt(var) + 1e-7;
        float* o = an + (size_t)role * 4 * Ch;
        o[tau] = bshift;
        o[Ch + tau] = (float)(1.0 / den);
        o[2 * Ch + tau] = (float)den;
        o[3 * Ch + tau] = (float)(-log(den));
    }
}

// ---- the same init from moments summed over ranks (data-parallel DDI) -------------------------------
// The reference lets its towers race on the assign (model.py:39 under train.py:43-57); here every rank adds its
// per-channel sum and sum of squares, the caller all-reduces the 4 Ch + 1 doubles (the last one counts rows), and
// every rank derives the same table: b = -mean, var((x + b)) = E[x^2] + 2 b E[x] + b^2 with the fp32-rounded b the
// single-process kernel above also centres with.
__global__ __launch_bounds__(256) void ddi_moments_kernel(const float* __restrict__ xa, const float* __restrict__ xb,
                                                          int M, int Ch, double* __restrict__ mom) {
    __shared__ double red[256];
    const int role = blockIdx.x / Ch, tau = blockIdx.x % Ch;
    const float* src = role ? xb : xa;
    double s = 0.0, s2 = 0.0;
    for (int r = threadIdx.x; r < M; r += 256) {
        const double v = src[(size_t)r * Ch + tau];
        s += v;
        s2 += v * v;
    }
    const double t1 = block_sum(s, red), t2 = block_sum(s2, red);
    if (threadIdx.x == 0) {
        mom[(size_t)role * 2 * Ch + tau] = t1;
        mom[(size_t)role * 2 * Ch + Ch + tau] = t2;
        if (blockIdx.x == 0) mom[4 * (size_t)Ch] = (double)M;
    }
}
__global__ void ddi_from_moments_kernel(const double* __restrict__ mom, int Ch, float* __restrict__ an) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * Ch) return;
    const int role = i / Ch, tau = i % Ch;
    const double n = mom[4 * (size_t)Ch];
    const double mean = mom[(size_t)role * 2 * Ch + tau] / n, ex2 = mom[(size_t)role * 2 * Ch + Ch + tau] / n;
    const float bshift = (float)(-mean);
    const double b = (double)bshift;
    const double var = fmax(ex2 + 2.0 * b * mean + b * b, 0.0);
    const double den = sqrt(var) + 1e-7;
    float* o = an + (size_t)role * 4 * Ch;
    o[tau] = bshift;
    o[Ch + tau] = (float)(1.0 / den);
    o[2 * Ch + tau] = (float)den;
    o[3 * Ch + tau] = (float)(-log(den));
}

// ---- ragged ActNorm init: one flow's moments over the clips' own rows -------------------------------------
// xa, xb [nclip][rows][Ch] fp32; clip c counts rows [0, len[c] / spr), clamped to the plane here: no row past a clip's end is
// loaded.  blockIdx.y = plane, blockIdx.x = chunk g of gridDim.x: the chunks stride over the rows of every clip, so a channel's
// sum is spread over gridDim.x workgroups (the plain kernel above gives a channel one workgroup: two in all at Ch = 1).
// part [gridDim.x][4 Ch] fp64 in mom's own layout; a chunk without a share leaves zeros.  Ch <= 256: a workgroup reads 256 / Ch
// whole rows per step (256 consecutive floats), thread t always channel t % Ch, and the threads of a channel are added pairwise
// in LDS.  Wider planes: one row per step, thread t channels t, t + 256, ...  Every order is fixed by the grid: no atomics.
__global__ __launch_bounds__(256) void ddi_moments_ragged_kernel(const float* __restrict__ xa, const float* __restrict__ xb,
                                                                 long nclip, long rows, int Ch, const int* __restrict__ len,
                                                                 int spr, double* __restrict__ part) {
    __shared__ double r1[256], r2[256];
    const int tid = threadIdx.x, role = blockIdx.y;
    const float* src = role ? xb : xa;
    double* out = part + ((size_t)blockIdx.x * 4 + 2 * role) * Ch;
    auto keep_of = [&](long c) { return clamp_len((long)len[c] / spr, rows); };
    if (Ch <= 256) {
        const int tau = tid & (Ch - 1), sub = tid / Ch, R = 256 / Ch;
        double s = 0.0, s2 = 0.0;
        for (long c = 0; c < nclip; ++c) {
            const long keep = keep_of(c);
            const float* p = src + (size_t)c * rows * Ch;
            for (long r = (long)blockIdx.x * R + sub; r < keep; r += (long)gridDim.x * R) {
                const double v = p[(size_t)r * Ch + tau];
                s += v;
                s2 += v * v;
            }
        }
        r1[tid] = s;
        r2[tid] = s2;
        __syncthreads();
        for (int st = 128; st >= Ch; st >>= 1) {             // tid and tid + st hold the same channel (st a multiple of Ch)
            if (tid < st) { r1[tid] += r1[tid + st]; r2[tid] += r2[tid + st]; }
            __syncthreads();
        }
        if (tid < Ch) { out[tau] = r1[tid]; out[Ch + tau] = r2[tid]; }
    } else {
        for (int tau = tid; tau < Ch; tau += 256) {
            double s = 0.0, s2 = 0.0;
            for (long c = 0; c < nclip; ++c) {
                const long keep = keep_of(c);
                const float* p = src + (size_t)c * rows * Ch;
                for (long r = blockIdx.x; r < keep; r += gridDim.x) {
                    const double v = p[(size_t)r * Ch + tau];
                    s += v;
                    s2 += v * v;
                }
            }
            out[tau] = s;
            out[Ch + tau] = s2;
        }
    }
}
// second stage: mom[i] = the chunks' part[g][i] added in index order, mom[4 Ch] = the number of rows counted
__global__ void ddi_moments_ragged_finish_kernel(const double* __restrict__ part, int nslot, long nclip, long rows, int Ch,
                                                 const int* __restrict__ len, int spr, double* __restrict__ mom) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 4 * Ch) {
        double s = 0.0;
        for (int g = 0; g < nslot; ++g) s += part[(size_t)g * 4 * Ch + i];
        mom[i] = s;
    } else if (i == 4 * Ch) {
        long n = 0;
        for (long c = 0; c < nclip; ++c) n += clamp_len((long)len[c] / spr, rows);
        mom[i] = (double)n;
    }
}

// ---- prior + log-det finalisation: out2 = (log_p, logdet), model.py:342-347 -----------------
__global__ __launch_bounds__(1024) void prior_kernel(const float* __restrict__ z, long n,
                                                     const float* __restrict__ partial, int n_partial,
                                                     double inv_bt, float* __restrict__ out2) {
    __shared__ double r1[1024], r2[1024];
    const int tid = threadIdx.x;
    double s = 0.0, p = 0.0;
    // eight loads in flight per thread, added in the same ascending order as one at a time (one dependent load per
    // iteration was a chain of n / 1024 memory round trips: 40 us for the bench batch, on the critical path of the pass)
    long i = tid;
    for (; i + 7 * 1024 < n; i += 8 * 1024) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = z[i + 1024L * u];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += (double)v[u] * (double)v[u];
    }
    for (; i < n; i += 1024) {
        const double v = z[i];
        s += v * v;
    }
    int j = tid;
    for (; j + 7 * 1024 < n_partial; j += 8 * 1024) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = partial[j + 1024 * u];
#pragma unroll
        for (int u = 0; u < 8; ++u) p += v[u];
    }
    for (; j < n_partial; j += 1024) p += partial[j];
    r1[tid] = s;
    r2[tid] = p;
    __syncthreads();
    for (int st = 512; st > 0; st >>= 1) {
        if (tid < st) { r1[tid] += r1[tid + st]; r2[tid] += r2[tid + st]; }
        __syncthreads();
    }
    if (tid == 0) {
        out2[0] = (float)(0.5 * (-1.8378770664093453 - r1[0] / (double)n));
        out2[1] = (float)(r2[0] * inv_bt);
    }
}

// ---- data-parallel optimiser step (train.py:15-32,75-81, utils.py:34-60) --------------------
// Gradients live in ONE flat fp32 buffer (what the RCCL all-reduce sums); the reference's
// average_gradients / un-scale / clip_by_global_norm / Adam chain becomes two HBM-bound passes:
//   (1) per-workgroup partial sums of g^2 (fixed order -> deterministic global norm),
//   (2) fused  g' = g * gscale / max(||g * gscale||, clip);  TF-form Adam on fp32 master weights.
__global__ __launch_bounds__(256) void sqnorm_partial_kernel(const float* __restrict__ g, long n,
                                                             double* __restrict__ partial) {
    __shared__ double red[256];
    double s = 0.0;
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (long)gridDim.x * 1024) {
        if (i + 3 < n) {
            const float4 v = *(const float4*)(g + i);
            s += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
        } else {
            for (long j = i; j < n; ++j) s += (double)g[j] * g[j];
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
// out[0] = sqrt(sum partial) * gscale  (= global norm of the averaged, un-scaled gradient)
__global__ __launch_bounds__(256) void sqnorm_final_kernel(const double* __restrict__ partial, int np,
                                                           float gscale, float* __restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < np; i += 256) s += partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)(sqrt(red[0]) * (double)gscale);
}
// tf.train.AdamOptimizer: lr_t = lr*sqrt(1-b2^t)/(1-b1^t); m,v updates; w -= lr_t*m/(sqrt(v)+eps)
__global__ __launch_bounds__(256) void adam_clip_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v, long n,
                                                        const float* __restrict__ gnorm, float gscale, float clip,
                                                        float lr_host, const float* __restrict__ lr_dev, float b1,
                                                        float b2, float eps) {
    const float lr_t = lr_dev ? lr_dev[0] : lr_host;     // device-resident rate: the launch can live in a hipGraph
    const float sc = gscale / fmaxf(gnorm[0], clip);     // tf.clip_by_global_norm: g / max(gn, clip)*clip, clip=1
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (long)gridDim.x * 1024) {
        if (i + 3 < n) {
            const float4 gv = *(const float4*)(g + i);
            float4 mv = *(float4*)(m + i), vv = *(float4*)(v + i), wv = *(float4*)(w + i);
            const float gg[4] = {gv.x * sc * clip, gv.y * sc * clip, gv.z * sc * clip, gv.w * sc * clip};
            float* mm = &mv.x; float* v2 = &vv.x; float* ww = &wv.x;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                mm[k] = b1 * mm[k] + (1.0f - b1) * gg[k];
                v2[k] = b2 * v2[k] + (1.0f - b2) * gg[k] * gg[k];
                ww[k] -= lr_t * mm[k] / (sqrtf(v2[k]) + eps);
            }
            *(float4*)(m + i) = mv; *(float4*)(v + i) = vv; *(float4*)(w + i) = wv;
        } else {
            for (long j = i; j < n; ++j) {
                const float gj = g[j] * sc * clip;
                m[j] = b1 * m[j] + (1.0f - b1) * gj;
                v[j] = b2 * v[j] + (1.0f - b2) * gj * gj;
                w[j] -= lr_t * m[j] / (sqrtf(v[j]) + eps);
            }
        }
    }
}
// Gradient accumulation: dst[i] = a ? a[i] + b[i] : b[i], one IEEE fp32 add per element.  dst may be a or b: every element is
// read and written by the same lane, so no pointer is __restrict__.  A block range of the flat layout starts at any element
// offset: `head` (0..3) scalar elements bring the three pointers to a 16-byte boundary when they share one misalignment, then
// nv float4s, then the scalar tail; pointers that do not share it come with head = 0, nv = 0 - the scalar loop over everything.
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* dst, const float* a, const float* b, long n, int head, long nv) {
    const long t0 = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    for (long q = t0; q < nv; q += stride) {
        const long i = head + 4 * q;
        float4 s = *(const float4*)(b + i);
        if (a) {
            const float4 av = *(const float4*)(a + i);
            s.x = av.x + s.x; s.y = av.y + s.y; s.z = av.z + s.z; s.w = av.w + s.w;
        }
        *(float4*)(dst + i) = s;
    }
    const long ns = n - 4 * nv;                          // the head in front of the float4 body and the tail behind it
    for (long s = t0; s < ns; s += stride) {
        const long i = s < head ? s : s + 4 * nv;
        dst[i] = a ? a[i] + b[i] : b[i];
    }
}

// ---- launchers -------------------------------------------------------------------------------
static inline int grid_for(long total) {
    long g = (total + 255) / 256;
    return (int)(g > 2048 ? 2048 : (g < 1 ? 1 : g));
}
void fwn_launch_wn_scale(const float* v, const float* g, int k_src, int n_src, float* scale, hipStream_t st) {
    hipLaunchKernelGGL(wn_scale_kernel, dim3((n_src + 31) / 32), dim3(1024), 0, st, v, g, k_src, n_src, scale);
}
void fwn_launch_pack(const float* v, const float* scale, const int* src_k, const int* src_n, int n_src,
                     int k_dst, int n_dst, long ld_dst, void* out, hipStream_t st) {
    const long total = (long)k_dst * n_dst;
    hipLaunchKernelGGL(pack_kernel, dim3(grid_for(total)), dim3(256), 0, st, v, scale, src_k, src_n, n_src,
                       k_dst, ld_dst, total, (bf16*)out);
}
void fwn_launch_upsample(const float* in, int B, int H, int W, const float* wk, float bias, const float* bias_dev, int s,
                         float* out_f32, void* out_planes, hipStream_t st) {
    const long total = (long)B * H * s * W;
    const bool al = (((uintptr_t)in | (uintptr_t)out_f32 | (uintptr_t)out_planes) & 15) == 0;
    if (W % 16 == 0 && al) {       // 8 bins per thread: whole 16-byte pieces in both mel halves
        hipLaunchKernelGGL(upsample8_kernel, dim3(grid_for(total / 8)), dim3(256), 0, st, in, B, H, W, wk, bias, bias_dev, s, out_f32,
                           (bf16*)out_planes);
        return;
    }
    hipLaunchKernelGGL(upsample_kernel, dim3(grid_for(total)), dim3(256), 0, st, in, B, H, W, wk, bias, bias_dev, s,
                       out_f32, (bf16*)out_planes);
}
void fwn_launch_split(const float* x, long B, long T, float* planes, hipStream_t st) {
    hipLaunchKernelGGL(split_kernel, dim3(grid_for(B * T)), dim3(256), 0, st, x, B, T, planes);
}
void fwn_launch_merge(const float* planes, long B, long T, float* x, hipStream_t st) {
    hipLaunchKernelGGL(merge_kernel, dim3(grid_for(B * T)), dim3(256), 0, st, planes, B, T, x);
}
void fwn_launch_mask_rows(void* base, long nclip, long rows, long row_bytes, const int* len, int nlen, int samples_per_row,
                          hipStream_t st) {
    hipLaunchKernelGGL(mask_rows_kernel, row_grid(rows * row_bytes, nclip), dim3(256), 0, st, (char*)base, rows, row_bytes, len, nlen,
                       samples_per_row);
}
void fwn_launch_pcm16(const float* x, short* pcm, long B, long T, const int* len, hipStream_t st) {
    hipLaunchKernelGGL(pcm16_kernel, row_grid(T * 2, B), dim3(256), 0, st, x, pcm, T, len);
}
void fwn_launch_latent_normal_at(float* z, long n, long L, unsigned long long seed, const unsigned* clip_id, const long long* start,
                                 float temp, const int* len, hipStream_t st) {
    hipLaunchKernelGGL(latent_normal_at_kernel, row_grid(L * 4, n), dim3(256), 0, st, z, L, (unsigned)(seed & 0xffffffffull),
                       (unsigned)(seed >> 32), clip_id, start, temp, len);
}
void fwn_launch_window_gather(const float* src, const long long* src_row, long row_floats, float* dst, long n, long count,
                              hipStream_t st) {
    hipLaunchKernelGGL(window_gather_kernel, row_grid(count * 4, n), dim3(256), 0, st, src, src_row, row_floats, dst, count);
}
void fwn_launch_window_scatter(const float* x, long n, long L, const int* core_off, const int* core_len, const long long* out_off,
                               short* pcm, float* wav, hipStream_t st) {
    hipLaunchKernelGGL(window_scatter_kernel, row_grid(L * (wav ? 4 : 2), n), dim3(256), 0, st, x, L, core_off, core_len, out_off, pcm,
                       wav);
}
void fwn_launch_corpus_draw(const float* audio, const float* mel, const long long* frame_off, long n_utt, int hop, int num_mels,
                            int unit_frames, long B, long F, unsigned long long seed, unsigned stream_id, unsigned long long* counter,
                            float* x, float* c, int* len, int* picks, hipStream_t st) {
    // sized for the longer of the two rows
    hipLaunchKernelGGL(corpus_draw_kernel, row_grid(F * (hop > num_mels ? hop : num_mels) * 4, B), dim3(256), 0, st, audio, mel, frame_off,
                       (unsigned long long)n_utt, hop, num_mels, unit_frames, F, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32),
                       stream_id, counter, x, c, len, picks);
    hipLaunchKernelGGL(corpus_advance_kernel, dim3(1), dim3(64), 0, st, counter);
}
void fwn_launch_fill_neg_shift(float* plane, long nclip, long rows, int Ch, const float* shift, const int* len, int nlen,
                               int samples_per_row, hipStream_t st) {
    hipLaunchKernelGGL(fill_neg_shift_kernel, row_grid(rows * Ch * 4, nclip), dim3(256), 0, st, plane, rows, Ch, shift, len, nlen,
                       samples_per_row);
}
// slots per clip and flow: up to 32 chunk sums (row_grid's cap over all clips) and the ActNorm term
int fwn_ragged_logdet_nslot(long nclip) {
    const long cap = row_cap(nclip);
    return (int)(cap > 32 ? 32 : cap) + 1;
}
void fwn_launch_range_logdet(const float* Z, long nclip, long rows, int Ch, const float* ez, const float* an, const int* off,
                             const int* cnt, int ncnt, int samples_per_row, double* acc, hipStream_t st) {
    const int nslot = fwn_ragged_logdet_nslot(nclip);
    hipLaunchKernelGGL(range_logdet_kernel, dim3((unsigned)(nslot - 1), (unsigned)nclip), dim3(256), 0, st, Z, rows, Ch, ez, an, off,
                       cnt, ncnt, samples_per_row, acc, nslot);
}
void fwn_launch_ragged_finish(const float* planes, long nclip, long T, const double* acc, int nflows, int n_flow, const int* len,
                              float* out2B, hipStream_t st) {
    hipLaunchKernelGGL(ragged_finish_kernel, dim3((unsigned)nclip), dim3(256), 0, st, planes, nclip, T, acc, nflows, n_flow,
                       fwn_ragged_logdet_nslot(nclip), len, out2B);
}
// windowed forward: one workgroup per window for its partial sums, row_grid for the latent, one lane per clip for
// the finish
void fwn_launch_window_sums(const float* planes, long n, long L, const int* core_off, const int* core_len, const double* acc,
                            int nflows, int n_flow, const int* slot, double* out, hipStream_t st) {
    hipLaunchKernelGGL(window_sums_kernel, dim3((unsigned)n), dim3(256), 0, st, planes, n, L, core_off, core_len, acc, nflows, n_flow,
                       fwn_ragged_logdet_nslot(n), slot, out);
}
void fwn_launch_window_latent(const float* planes, long n, long L, int swapped, const int* core_off, const int* core_len,
                              const long long* out_off, float* z, hipStream_t st) {
    hipLaunchKernelGGL(window_latent_kernel, row_grid(L * 4, n), dim3(256), 0, st, planes, n, L, swapped, core_off, core_len, out_off, z);
}
void fwn_launch_windows_finish(const double* part, const int* slot0, const int* nwin, long nclip, float* out2B, hipStream_t st) {
    hipLaunchKernelGGL(windows_finish_kernel, dim3((unsigned)((nclip + 63) / 64)), dim3(64), 0, st, part, slot0, nwin, nclip, out2B);
}
void fwn_launch_ddi_moments(const float* xa, const float* xb, int M, int Ch, double* mom, hipStream_t st) {
    hipLaunchKernelGGL(ddi_moments_kernel, dim3(2 * Ch), dim3(256), 0, st, xa, xb, M, Ch, mom);
}
void fwn_launch_ddi_from_moments(const double* mom, int Ch, float* an, hipStream_t st) {
    hipLaunchKernelGGL(ddi_from_moments_kernel, dim3((2 * Ch + 63) / 64), dim3(64), 0, st, mom, Ch, an);
}
void fwn_launch_ddi(const float* xa, const float* xb, int M, int Ch, float* an, hipStream_t st) {
    hipLaunchKernelGGL(ddi_kernel, dim3(2 * Ch), dim3(256), 0, st, xa, xb, M, Ch, an);
}
// chunks of the ragged moments: about 4096 elements of a plane each, 64 at most (the shape decides, not the lengths)
int fwn_ragged_moments_nslot(long nclip, long rows, int Ch) {
    const long want = nclip * rows * Ch / 4096;
    return (int)(want < 1 ? 1 : (want > 64 ? 64 : want));
}
void fwn_launch_ddi_moments_ragged(const float* xa, const float* xb, long nclip, long rows, int Ch, const int* len,
                                   int samples_per_row, double* mom, double* part, hipStream_t st) {
    const int nslot = fwn_ragged_moments_nslot(nclip, rows, Ch);
    hipLaunchKernelGGL(ddi_moments_ragged_kernel, dim3((unsigned)nslot, 2), dim3(256), 0, st, xa, xb, nclip, rows, Ch, len,
                       samples_per_row, part);
    hipLaunchKernelGGL(ddi_moments_ragged_finish_kernel, dim3((4 * Ch + 1 + 63) / 64), dim3(64), 0, st, part, nslot, nclip, rows, Ch,
                       len, samples_per_row, mom);
}
void fwn_launch_prior(const float* planes, long n, const float* partial, int n_partial, double inv_bt,
                      float* out2, hipStream_t st) {
    hipLaunchKernelGGL(prior_kernel, dim3(1), dim3(1024), 0, st, planes, n, partial, n_partial, inv_bt, out2);
}

// ---- mel front-end: wav -> normalised log-mel frames (preprocessing.py:58-69) --------------------
// One workgroup per (frame, clip): centred reflect-padded frame x periodic Hann window -> direct
// DFT (the window is 1024 points and a 10 s clip has 862 frames: an FFT would buy microseconds)
// -> |.|^2 -> mel filterbank -> 20 log10(max(1e-4, .)) - ref -> clip((. - min) / -min, 0, 1).
// The 20 log10 of a POWER spectrum is the reference's (preprocessing.py:67) and kept.
__global__ __launch_bounds__(256) void mel_kernel(const float* __restrict__ wav, long T, int frames,
                                                  const float* __restrict__ window, const float* __restrict__ fb,
                                                  int n_fft, int hop, int n_mels, float ref_db, float min_db,
                                                  float* __restrict__ mel) {
    extern __shared__ float sm[];
    float* xw = sm;                    // [n_fft] windowed frame
    float* cs = xw + n_fft;            // [n_fft] cos(2 pi j / n_fft)
    float* sn = cs + n_fft;            // [n_fft] sin(2 pi j / n_fft)
    float* pw = sn + n_fft;            // [n_fft/2 + 1] power spectrum
    const int fr = blockIdx.x, nb = n_fft / 2 + 1;
    const float* y = wav + (long)blockIdx.y * T;
    for (int n = threadIdx.x; n < n_fft; n += 256) {
        long j = (long)fr * hop + n - n_fft / 2;
        if (j < 0) j = -j;                         // numpy 'reflect': the edge sample is not repeated
        if (j >= T) j = 2 * (T - 1) - j;
        xw[n] = y[j] * window[n];
        float sv, cv;
        sincospif(2.0f * (float)n / (float)n_fft, &sv, &cv);
        cs[n] = cv;
        sn[n] = sv;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nb; k += 256) {
        float re = 0.0f, im = 0.0f;
        int idx = 0;
        for (int n = 0; n < n_fft; ++n) {
            re = fmaf(xw[n], cs[idx], re);
            im = fmaf(-xw[n], sn[idx], im);
            idx = (idx + k) & (n_fft - 1);
        }
        pw[k] = re * re + im * im;
    }
    __syncthreads();
    for (int m = threadIdx.x; m < n_mels; m += 256) {
        const float* w = fb + (long)m * nb;
        float acc = 0.0f;
        for (int k = 0; k < nb; ++k) acc = fmaf(w[k], pw[k], acc);
        const float db = 20.0f * log10f(fmaxf(1e-4f, acc)) - ref_db;
        mel[((long)blockIdx.y * frames + fr) * n_mels + m] = fminf(fmaxf((db - min_db) / (-min_db), 0.0f), 1.0f);
    }
}
void fwn_launch_mel(const float* wav, long B, long T, const float* window, const float* fb, int n_fft, int hop,
                    int n_mels, float ref_db, float min_db, float* mel, hipStream_t st) {
    const int frames = (int)(1 + T / hop);
    const size_t lds = (size_t)(3 * n_fft + n_fft / 2 + 1) * sizeof(float);
    hipLaunchKernelGGL(mel_kernel, dim3(frames, (unsigned)B), dim3(256), lds, st, wav, T, frames, window, fb,
                       n_fft, hop, n_mels, ref_db, min_db, mel);
}

int fwn_sqnorm_blocks(long n) { long b = (n + 1023) / 1024; return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b)); }
void fwn_launch_grad_norm(const float* g, long n, float gscale, double* partial, float* out, hipStream_t st) {
    const int nb = fwn_sqnorm_blocks(n);
    hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(nb), dim3(256), 0, st, g, n, partial);
    hipLaunchKernelGGL(sqnorm_final_kernel, dim3(1), dim3(256), 0, st, partial, nb, gscale, out);
}
void fwn_launch_adam(float* w, const float* g, float* m, float* v, long n, const float* gnorm, float gscale,
                     float clip, float lr_t, const float* lr_dev, float b1, float b2, float eps, hipStream_t st) {
    hipLaunchKernelGGL(adam_clip_kernel, dim3(fwn_sqnorm_blocks(n)), dim3(256), 0, st, w, g, m, v, n, gnorm, gscale,
                       clip, lr_t, lr_dev, b1, b2, eps);
}
void fwn_launch_grad_accumulate(float* dst, const float* a, const float* b, long n, hipStream_t st) {
    const unsigned mis = (unsigned)((uintptr_t)dst & 15);
    const bool same = ((uintptr_t)b & 15) == mis && (!a || ((uintptr_t)a & 15) == mis);
    long head = same ? (long)((16 - mis) & 15) / 4 : 0;
    if (head > n) head = n;
    const long nv = same ? (n - head) / 4 : 0;
    hipLaunchKernelGGL(grad_accumulate_kernel, dim3(fwn_sqnorm_blocks(n)), dim3(256), 0, st, dst, a, b, n, (int)head, nv);
}
