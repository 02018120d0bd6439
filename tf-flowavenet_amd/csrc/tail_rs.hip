// Translation unit of the register-streamed tail (tail_rs.h): the kernel's instantiations and the fragment-stream packing (the
// rows it serves: fwn_tail_form in flow_kernels.hip).  Its own unit so that it builds beside flow_kernels.hip (four minutes of hipcc).
#include "tail_rs.h"
#include "fwn_internal.h"

// bytes of the fragment stream of one flow (Wskip | Wfinal), 0: no kernel for this layer count
long fwn_tail_stream_size(int L) { return L == 2 ? 8L * 48 * 1024 : 0; }

void fwn_launch_tail_stream_pack(const void* Ws, const void* Wf, void* out, hipStream_t st) {
    hipLaunchKernelGGL(tail_stream_pack_kernel, dim3(96), dim3(256), 0, st, (const bf16*)Ws, (const bf16*)Wf, (bf16*)out, (const TailStreamJob*)nullptr);
}
void fwn_launch_tail_stream_pack_jobs(const void* jobs, int njobs, hipStream_t st) {
    hipLaunchKernelGGL(tail_stream_pack_kernel, dim3(24, njobs), dim3(256), 0, st, (const bf16*)nullptr, (const bf16*)nullptr, (bf16*)nullptr,
                       (const TailStreamJob*)jobs);
}

void fwn_launch_tail_rs(const TailArgs& a, const void* Wts, int mt, hipStream_t st) {
    const bool front = a.h0_next != nullptr, save = a.save_s && a.save_u && a.save_z;
    const int rows = 32 * mt - (a.overlap ? 2 : 0);
    const dim3 grid((a.M + rows - 1) / rows), block(512);
#define TRS_LAUNCH(MT)                                                                                                       \
    do {                                                                                                                     \
        if (front) hipLaunchKernelGGL((tail_rs_kernel<MT, true, false>), grid, block, 0, st, a, (const bf16*)Wts);           \
        else if (save) hipLaunchKernelGGL((tail_rs_kernel<MT, false, true>), grid, block, 0, st, a, (const bf16*)Wts);       \
        else hipLaunchKernelGGL((tail_rs_kernel<MT, false, false>), grid, block, 0, st, a, (const bf16*)Wts);                \
    } while (0)
    if (mt == 4) TRS_LAUNCH(4);
    else if (mt == 2) TRS_LAUNCH(2);
    else TRS_LAUNCH(1);
#undef TRS_LAUNCH
}
