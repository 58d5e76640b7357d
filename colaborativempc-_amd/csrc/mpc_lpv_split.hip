// The stable partition of a batch by the detector's level (include/cmpc.h, cmpc_mpc_lpv_split_dev; the second launch
// of CMPC_FLAG_LPV_SPLIT): conf <- the agents with level > 0, rest <- the others, both ascending, each list's count
// at index batch.  The v3 kernel's two instantiations then take their agents from the lists (MpcPtrs::alist).
//
// One 1024-thread workgroup, as the polish launch's list (mpc_polish.hip, polish_list_kernel): a ballot per wave,
// the waves' counts summed through LDS, 1024 agents per step.  Both lists come out of the same pass: the agents
// below b that are not in conf are in rest, so b's rest slot is b minus its conf offset.  Every store is an
// ordinary vector store; entries past a list's count are not written.
#include "internal.h"

namespace cmpc {

namespace {

constexpr int kSplitBlock = 1024;

__global__ __launch_bounds__(kSplitBlock) void lpv_split_kernel(const int* __restrict__ level, int batch,
                                                                 int* __restrict__ conf, int* __restrict__ rest) {
    __shared__ int cnt[kSplitBlock / kWave];
    const int tid = threadIdx.x, wv = tid >> 6, l = tid & 63;
    int base = 0;  // conforming agents below b0
    for (int b0 = 0; b0 < batch; b0 += kSplitBlock) {
        const int b = b0 + tid;
        const bool in = b < batch;
        const bool on = in && level[b] > 0;
        const unsigned long long msk = __ballot(on);
        if (l == 0) cnt[wv] = __popcll(msk);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wv; ++w) off += cnt[w];
        off += __popcll(msk & ((1ull << l) - 1ull));  // conforming agents below b: 0 <= off <= b
        if (on) conf[off] = b;
        else if (in) rest[b - off] = b;
        for (int w = 0; w < kSplitBlock / kWave; ++w) base += cnt[w];
        __syncthreads();
    }
    if (tid == 0) {
        conf[batch] = base;
        rest[batch] = batch - base;
    }
}

}  // namespace

hipError_t mpc_lpv_split_launch(int batch, const int* level, int* conf, int* rest, hipStream_t s) {
    if (batch <= 0) return hipSuccess;
    hipLaunchKernelGGL(lpv_split_kernel, dim3(1), dim3(kSplitBlock), 0, s, level, batch, conf, rest);
    return hipGetLastError();
}

}  // namespace cmpc
