// Reference structure detected on the device (include/cmpc.h, cmpc_mpc_lpv_level[_dev]): which agents of an
// eligible batch (nx 9, nu 2, mc = 4 + nb) hold the pattern under which the v3 kernel's compact (LS) load applies —
//   A_k = I outside columns 0..2, B_k = 0 outside rows 0..2,
//   rows 0, 1 on vx (column 0) only, rows 2, 3 on ey (column 3) only, rows 4.. on (X, Y) (columns 7, 8) only
// — exactly the entries mpc_ipm3.hip's LS staging never reads.  Eligibility (dimensions, row tables, Q diagonal,
// flags) is the host's: mpc_lpv_eligible.
//
// A streaming kernel: one 256-thread workgroup per agent reads that agent's A, B and C once (N (81 + 18 + 9 mc)
// doubles, 36 KB at N = 30, mc = 6), consecutive threads consecutive addresses, four loads in flight per thread.
// Every thread ORs its violations into one flag; a wave ballot and four LDS words combine them; thread 0 writes
// the agent's level and counts a nonconforming agent with one vector atomic.  Values are tested on their bits
// (|x| == 0 is "all bits but the sign clear", x == 1 is the one pattern 0x3ff0...0), which is the comparison by
// value of cmpc.h — -0.0 conforms, NaN and denormals do not — whatever the wave's denormal mode.
#include "internal.h"

namespace cmpc {

namespace {

constexpr int kDetBlock = 256;
constexpr unsigned long long kAbsMask = 0x7fffffffffffffffull;
constexpr unsigned long long kOneBits = 0x3ff0000000000000ull;

__device__ __forceinline__ unsigned long long bits_of(const double* p, size_t i) {
    return (unsigned long long)__double_as_longlong(p[i]);
}

// 1 when entry q (row-major index in a 9 x 9 stage block) of A breaks the pattern
struct BadA {
    __device__ __forceinline__ unsigned operator()(unsigned long long v, int q) const {
        const int r = q / 9, t = q - r * 9;
        if (t < 3) return 0u;
        return r == t ? (v != kOneBits) : ((v & kAbsMask) != 0ull);
    }
};
// ... entry q of a 9 x 2 stage block of B: rows 3.. are zero
struct BadB {
    __device__ __forceinline__ unsigned operator()(unsigned long long v, int q) const {
        return q >= 6 && (v & kAbsMask) != 0ull;
    }
};
// ... entry q of an mc x 9 stage block of C
struct BadC {
    __device__ __forceinline__ unsigned operator()(unsigned long long v, int q) const {
        const int r = q / 9, col = q - r * 9;
        const bool read = r < 2 ? col == 0 : (r < 4 ? col == 3 : col >= 7);
        return !read && (v & kAbsMask) != 0ull;
    }
};

template <class F>
__device__ __forceinline__ unsigned scan(const double* g, int count, int per, F bad) {
    unsigned any = 0u;
    int i = threadIdx.x;
    // four independent loads per trip keep the memory pipe busy from one wave
    for (; i + 3 * kDetBlock < count; i += 4 * kDetBlock) {
        const unsigned long long v0 = bits_of(g, i), v1 = bits_of(g, i + kDetBlock), v2 = bits_of(g, i + 2 * kDetBlock),
                                 v3 = bits_of(g, i + 3 * kDetBlock);
        any |= bad(v0, i % per) | bad(v1, (i + kDetBlock) % per) | bad(v2, (i + 2 * kDetBlock) % per) |
               bad(v3, (i + 3 * kDetBlock) % per);
    }
    for (; i < count; i += kDetBlock) any |= bad(bits_of(g, i), i % per);
    return any;
}

__global__ __launch_bounds__(kDetBlock) void lpv_detect_kernel(int N, int mc, int qlevel, const double* A,
                                                                const double* B, const double* C, int* level,
                                                                int* noncon) {
    __shared__ unsigned flag[kDetBlock / kWave];
    const size_t b = blockIdx.x;
    unsigned any = scan(A + b * (size_t)N * 81, N * 81, 81, BadA{});
    any |= scan(B + b * (size_t)N * 18, N * 18, 18, BadB{});
    any |= scan(C + b * (size_t)N * mc * 9, N * mc * 9, mc * 9, BadC{});
    const unsigned long long vote = __ballot(any != 0u);
    if ((threadIdx.x & (kWave - 1)) == 0) flag[threadIdx.x / kWave] = vote != 0ull;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned f = 0u;
        for (int w = 0; w < kDetBlock / kWave; ++w) f |= flag[w];
        if (level) level[b] = f ? 0 : qlevel;
        if (noncon && f) atomicAdd(noncon, 1);
    }
}

}  // namespace

int mpc_lpv_eligible(const MpcConst& c, int flags) {
    if (flags & (CMPC_FLAG_GENERIC | CMPC_FLAG_RICCATI | CMPC_FLAG_LANE | CMPC_FLAG_FP32)) return 0;
    if (c.nx != 9 || c.nu != 2 || c.ns != 3 || c.mc < 4 || c.mc > 7 || c.N > 32 || c.n > 64) return 0;
    // the v3 row tables (mpc_ipm3.hip slk / sgn)
    const int base_slack[4] = {-1, 0, 1, 1};
    for (int r = 0; r < c.mc; ++r)
        if (c.row_slack[r] != (r < 4 ? base_slack[r] : 2) || c.row_sign[r] != (r < 4 ? 1 : -1)) return 0;
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j)
            if (i != j && c.Q[i * 9 + j] != 0.0) return 0;
    // 2: Q also zero on states 1, 2, 5, 6: the LS kernel's L5 contraction
    return (c.Q[1 * 9 + 1] == 0.0 && c.Q[2 * 9 + 2] == 0.0 && c.Q[5 * 9 + 5] == 0.0 && c.Q[6 * 9 + 6] == 0.0) ? 2 : 1;
}

hipError_t mpc_lpv_detect_launch(const MpcConst& c, int qlevel, const double* A, const double* B, const double* C,
                                 int* level, int* noncon, int batch, hipStream_t s) {
    if (batch <= 0) return hipSuccess;
    if (noncon) {
        const hipError_t e = hipMemsetAsync(noncon, 0, sizeof(int), s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lpv_detect_kernel, dim3((unsigned)batch), dim3(kDetBlock), 0, s, c.N, c.mc, qlevel, A, B, C,
                       level, noncon);
    return hipGetLastError();
}

}  // namespace cmpc
