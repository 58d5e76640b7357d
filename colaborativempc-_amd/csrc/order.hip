// Launch order on the device (include/cmpc.h, cmpc_order_by_iters_dev): the agents by descending
// key(b) = min(max(iters[b], 0), 65535), ties by ascending index — the permutation cmpc_opts.order takes
// (longest solves first), so a host without torch can build it between two rounds without leaving the stream.
//
// Shape: a stable least-significant-digit radix sort of (65535 - key, index), two passes on 8-bit digits, by
// ONE workgroup of up to 1024 threads that walks the batch in tiles of its size, in index order (correct for
// any batch; cfg5's 8192 agents are 8 tiles).  One read of iters counts both digits' histograms (LDS atomics:
// a count does not depend on the order of its additions); an exclusive scan turns them into the digits' bases.
// A pass then places every element at  base[digit] + its rank among the equal digits before it:  inside a
// wavefront the rank is the popcount of the lower lanes of the digit's match mask (eight __ballot masks, one
// per digit bit) — never an LDS atomic, whose return order is arbitrary and would lose the stable order; across
// the tile's wavefronts it is a 256-wide scan over their per-digit counts, which also advances the bases to the
// next tile.  Pass 1 writes (65535 - key, index) pairs to a scratch array, pass 2 reads them back in that order
// and writes the indices.  No workgroup ever waits on another: there is only one.
#include "internal.h"

namespace cmpc {

namespace {

constexpr int kOrdThreads = 1024;              // the workgroup's capacity; a smaller batch launches fewer
constexpr int kOrdWaves = kOrdThreads / kWave;
constexpr int kOrdDigits = 256;

__device__ __forceinline__ unsigned ord_key(int it) { return 65535u - (unsigned)min(max(it, 0), 65535); }

// hist[0..256) -> its exclusive prefix sums, by one wavefront (lane l owns digits 4l .. 4l + 3)
__device__ __forceinline__ void ord_scan(int* hist, int lane) {
    const int4 v = reinterpret_cast<int4*>(hist)[lane];
    const int own = v.x + v.y + v.z + v.w;
    int inc = own;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int up = __shfl_up(inc, d, kWave);
        if (lane >= d) inc += up;
    }
    const int e = inc - own;
    reinterpret_cast<int4*>(hist)[lane] = int4{e, e + v.x, e + v.x + v.y, e + v.x + v.y + v.z};
}

// One stable pass over a tile: `digit` of this thread's element (valid: the thread has one) -> its position.
// base[d]: where the tile's first element of digit d goes; advanced past the tile on return.
__device__ __forceinline__ int ord_place(bool valid, unsigned digit, int* base, int (*wc)[kOrdDigits], int lane, int w,
                                         int nw) {
    // no wavefront still reads the previous tile's counts (the barrier that ended the previous call)
    for (int i = threadIdx.x; i < nw * kOrdDigits / 4; i += blockDim.x) reinterpret_cast<int4*>(wc)[i] = int4{0, 0, 0, 0};
    unsigned long long peers = __ballot(valid);  // the lanes of this wavefront that hold the same digit
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
        const bool one = (digit >> bit) & 1u;
        const unsigned long long m = __ballot(valid && one);
        peers &= one ? m : ~m;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));  // equal digits in lower lanes = earlier indices
    __syncthreads();
    if (valid && rank == 0) wc[w][digit] = __popcll(peers);
    __syncthreads();
    // digit d: the wavefronts' counts -> their bases, in wavefront (= index) order (a small batch launches
    // fewer threads than digits)
    for (int d = threadIdx.x; d < kOrdDigits; d += blockDim.x) {
        int run = base[d];
        for (int i = 0; i < nw; ++i) {
            const int t = wc[i][d];
            wc[i][d] = run;
            run += t;
        }
        base[d] = run;
    }
    __syncthreads();
    const int pos = valid ? wc[w][digit] + rank : -1;
    __syncthreads();
    return pos;
}

// tmp is written in pass 1 and read in pass 2 by other threads of the same workgroup: no __restrict__ on it
__global__ __launch_bounds__(kOrdThreads) void order_kernel(int batch, const int* __restrict__ iters,
                                                            int* __restrict__ order, unsigned long long* tmp) {
    __shared__ __attribute__((aligned(16))) int base[2][kOrdDigits];
    __shared__ __attribute__((aligned(16))) int wc[kOrdWaves][kOrdDigits];
    const int lane = threadIdx.x & (kWave - 1);
    const int w = threadIdx.x / kWave, nw = blockDim.x / kWave;

    for (int i = threadIdx.x; i < 2 * kOrdDigits; i += blockDim.x) base[0][i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < batch; i += blockDim.x) {
        const unsigned k = ord_key(iters[i]);
        atomicAdd(&base[0][k & 255u], 1);
        atomicAdd(&base[1][k >> 8], 1);
    }
    __syncthreads();
    if (w == 0) {
        ord_scan(base[0], lane);
        ord_scan(base[1], lane);
    }
    __syncthreads();

    for (int t0 = 0; t0 < batch; t0 += blockDim.x) {  // pass 1: by the low digit, input in index order
        const int i = t0 + threadIdx.x;
        const bool valid = i < batch;
        const unsigned k = valid ? ord_key(iters[i]) : 0u;
        const int pos = ord_place(valid, k & 255u, base[0], wc, lane, w, nw);
        if (valid && (unsigned)pos < (unsigned)batch) tmp[pos] = ((unsigned long long)k << 32) | (unsigned)i;
    }
    __threadfence_block();
    __syncthreads();
    for (int t0 = 0; t0 < batch; t0 += blockDim.x) {  // pass 2: by the high digit, input in pass 1's order
        const int i = t0 + threadIdx.x;
        const bool valid = i < batch;
        const unsigned long long e = valid ? tmp[i] : 0ull;
        const int pos = ord_place(valid, (unsigned)(e >> 40) & 255u, base[1], wc, lane, w, nw);
        if (valid && (unsigned)pos < (unsigned)batch) order[pos] = (int)(unsigned)e;
    }
}

}  // namespace

hipError_t order_launch(int batch, const int* iters, int* order, unsigned long long* tmp, hipStream_t s) {
    if (batch <= 0) return hipSuccess;
    const int threads = batch >= kOrdThreads ? kOrdThreads : (batch + kWave - 1) / kWave * kWave;
    hipLaunchKernelGGL(order_kernel, dim3(1), dim3(threads), 0, s, batch, iters, order, tmp);
    return hipGetLastError();
}

}  // namespace cmpc
