// Neighbour selection on the device (include/cmpc.h, cmpc_nbr_select_dev): for every local agent the nb
// nearest other agents out of the n_total trajectories of the exchange buffer, so a consensus round can
// rebuild its neighbour table without the host (the reference fixes ns[i] once, LPV_HP_N_main.py:82-85).
//
//   score(g, j) = min over k in [k0, k1] of (dx dx + dy dy),  dx = traj_all[j, k, 0] - traj_all[g, k, 0]
//   (numpy's min: NaN at any stage of the window makes the score NaN), a NaN score counts as +inf;
//   candidates ordered by (score, j) ascending, j = g left out by index; output nearest first.
//
// Shape: one wavefront per local agent, WAVES (4 or 8) agents per workgroup.  The workgroup walks the
// candidates in tiles of kSelTile (each lane owns kSelPerLane of them) and the window in chunks of
// kSelChunk stages: a chunk of a tile is staged once in LDS, stage-major so a lane's 16-byte read is
// conflict-free, and read by all of the workgroup's agents.  The next chunk's global loads are issued
// into registers before the current chunk is scored, so their latency overlaps the arithmetic.  Each
// lane keeps the NBC best (score, j) pairs it has seen, sorted, in registers; the wave's result is a
// merge of nb wave-wide lexicographic arg-mins over the lanes' list heads (DPP reductions of
// wave_ops.h).  Each expression is evaluated without fma contraction, so a score has the bits of
// numpy's dx*dx + dy*dy.
#include <climits>

#include "internal.h"
#include "wave_ops.h"

namespace cmpc {

namespace {

// agents (wavefronts) per workgroup, the template parameter WAVES: each shares the staged candidates, so a
// workgroup of WAVES agents reads the whole window of every candidate once from L2.  4 spreads a population of
// up to kSelWideBatch agents over more compute units; from there on 8 halves the L2 traffic that bounds a
// long window at such sizes
constexpr int kSelWideBatch = 2048;
constexpr int kSelPerLane = 2;                        // candidates per lane and tile
constexpr int kSelTile = kWave * kSelPerLane;         // candidates per tile
constexpr int kSelChunk = 16;                         // stages per LDS chunk
constexpr int kSelLd = kSelTile + 1;                  // padded row of the stage-major tile (staging stores)
constexpr int sel_stage(int waves) { return kSelTile * kSelChunk / (waves * kWave); }  // a thread's share of a chunk

// (s, j) < (bs, bj); every s is a number or +inf here
__device__ __forceinline__ bool sel_less(double s, int j, double bs, int bj) { return s < bs || (s == bs && j < bj); }

// One thread's share of a chunk (kc stages of the tile's candidates) on its way from global memory to LDS.
// Element i = thread + e * (threads of the workgroup) is stage i % kc of candidate i / kc: consecutive threads take
// consecutive stages of one candidate (kc * 16 contiguous bytes); a one-stage window is the strided gather,
// one candidate per thread.
template <int WAVES>
struct SelFetch {
    double2 v[sel_stage(WAVES)];
    double2 own;   // lane l: the wave's own agent at stage l of the chunk
    int jj, kk;    // element 0 of this thread
};

// calls f(e, jj, kk) for this thread's elements inside the step's `span` candidates; one division, then carries
template <int WAVES, class F>
__device__ __forceinline__ void sel_walk(int jj, int kk, int kc, int span, F&& f) {
    static_assert(sel_stage(WAVES) * WAVES * kWave == kSelTile * kSelChunk, "a full chunk divides among the threads");
    const int dj = WAVES * kWave / kc, dk = WAVES * kWave - dj * kc;
#pragma unroll
    for (int e = 0; e < sel_stage(WAVES); ++e) {
        if (jj < span) f(e, jj, kk);
        jj += dj;
        kk += dk;
        if (kk >= kc) {
            kk -= kc;
            ++jj;
        }
    }
}

template <int WAVES>
__device__ __forceinline__ void sel_fetch(const NbrConst& c, const double* __restrict__ traj_all, int g, int lane,
                                          int j0, int kc0, int kc, int span, SelFetch<WAVES>& f) {
    const size_t row = (size_t)(c.N + 1) * 2;
    f.jj = threadIdx.x / kc;
    f.kk = threadIdx.x - f.jj * kc;
    sel_walk<WAVES>(f.jj, f.kk, kc, span, [&](int e, int jj, int kk) {
        double2 v = {0.0, 0.0};  // past the population: never selected (j < n_total at the insertion)
        if (j0 + jj < c.n_total) {
            const double* p = traj_all + (size_t)(j0 + jj) * row + (size_t)(kc0 + kk) * 2;
            v.x = p[0];
            v.y = p[1];
        }
        f.v[e] = v;
    });
    if (lane < kc) {
        const double* p = traj_all + (size_t)g * row + (size_t)(kc0 + lane) * 2;
        f.own = double2{p[0], p[1]};
    }
}

// Running min over the chunk's stages for this lane's candidates.  numpy's min keeps a NaN; fmin drops it, so
// the stages are also summed: every d is >= 0, +inf or NaN, and such a sum is NaN exactly when a term is
// (one add per stage instead of two compares and a select).
template <bool FULL>
__device__ __forceinline__ void sel_score(const double2 (*tile)[kSelLd], const double2* own, int lane, int kc,
                                          double (&run)[kSelPerLane], double (&sum)[kSelPerLane]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int kk = 0; kk < (FULL ? kSelChunk : kc); ++kk) {
        const double2 o = own[kk];
#pragma unroll
        for (int m = 0; m < kSelPerLane; ++m) {
            const double2 q = tile[kk][m * kWave + lane];
            const double dx = q.x - o.x, dy = q.y - o.y;
            const double d = dx * dx + dy * dy;
            run[m] = fmin(run[m], d);
            sum[m] = sum[m] + d;
        }
    }
}

template <int NBC, int WAVES>
__global__ __launch_bounds__(WAVES* kWave) void nbr_select_kernel(NbrConst c, const double* __restrict__ traj_all,
                                                                  int* __restrict__ nbr, double* __restrict__ dist2) {
    __shared__ double2 tile[kSelChunk][kSelLd];
    __shared__ double2 own[WAVES][kSelChunk];
    const int lane = threadIdx.x & (kWave - 1);
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int b = blockIdx.x * WAVES + w;
    const bool live = b < c.batch;  // wave-uniform; a wave past the batch still helps staging
    const int g = c.self_offset + (live ? b : c.batch - 1);
    const double inf = __builtin_inf();

    double ls[NBC];  // this lane's best candidates so far, ascending by (score, j)
    int lj[NBC];
#pragma unroll
    for (int i = 0; i < NBC; ++i) {
        ls[i] = inf;
        lj[i] = INT_MAX;
    }
    double run[kSelPerLane], sum[kSelPerLane];  // min and sum over the window's stages so far
#pragma unroll
    for (int m = 0; m < kSelPerLane; ++m) {
        run[m] = inf;
        sum[m] = 0.0;
    }

    // A step stages kc stages of `span` candidates: one tile while the window takes several chunks; a window
    // of W <= kSelChunk stages leaves room for kSelChunk / W tiles side by side (rows t * kc + kk), so a
    // one-stage window moves 16 tiles per step instead of paying a global round trip and two barriers for
    // each.  j0 / kc0: the current step's; nj0 / nkc0: the one being fetched.
    const int W = c.k1 - c.k0 + 1;
    const int nt = W <= kSelChunk ? kSelChunk / W : 1, span = nt * kSelTile;
    SelFetch<WAVES> f;
    int j0 = 0, kc0 = c.k0;
    sel_fetch(c, traj_all, g, lane, j0, kc0, min(kSelChunk, W), span, f);
    while (j0 < c.n_total) {
        const int kc = min(kSelChunk, c.k1 + 1 - kc0);
        __syncthreads();  // the previous step has been read
        sel_walk<WAVES>(f.jj, f.kk, kc, span,
                        [&](int e, int jj, int kk) { tile[(jj / kSelTile) * kc + kk][jj % kSelTile] = f.v[e]; });
        if (lane < kc) own[w][lane] = f.own;
        __syncthreads();
        const bool last = kc0 + kc > c.k1;  // the window's last chunk: the scores are complete
        const int nj0 = last ? j0 + span : j0, nkc0 = last ? c.k0 : kc0 + kc;
        if (nj0 < c.n_total) sel_fetch(c, traj_all, g, lane, nj0, nkc0, min(kSelChunk, c.k1 + 1 - nkc0), span, f);
        for (int t = 0; t < nt && j0 + t * kSelTile < c.n_total; ++t) {
            if (kc == kSelChunk)
                sel_score<true>(tile + t * kc, own[w], lane, kc, run, sum);
            else
                sel_score<false>(tile + t * kc, own[w], lane, kc, run, sum);
            if (!last) continue;
#pragma unroll
            for (int m = 0; m < kSelPerLane; ++m) {
                const int j = j0 + t * kSelTile + m * kWave + lane;
                const double s = sum[m] != sum[m] ? inf : run[m];  // a NaN score counts as +inf
                run[m] = inf;
                sum[m] = 0.0;
                if (j < c.n_total && j != g && sel_less(s, j, ls[NBC - 1], lj[NBC - 1])) {
                    bool lt[NBC];
#pragma unroll
                    for (int i = 0; i < NBC; ++i) lt[i] = sel_less(s, j, ls[i], lj[i]);
#pragma unroll
                    for (int i = NBC - 1; i > 0; --i) {
                        ls[i] = lt[i - 1] ? ls[i - 1] : (lt[i] ? s : ls[i]);
                        lj[i] = lt[i - 1] ? lj[i - 1] : (lt[i] ? j : lj[i]);
                    }
                    ls[0] = lt[0] ? s : ls[0];
                    lj[0] = lt[0] ? j : lj[0];
                }
            }
        }
        j0 = nj0;
        kc0 = nkc0;
    }

    // merge: nb times the wave's smallest list head by (score, j); its lane moves on to its next entry.
    // Every candidate sits in exactly one lane, and nb < n_total, so the winner is one lane's real entry.
    for (int r = 0; r < c.nb; ++r) {
        const double smin = wave_min(ls[0]);
        const double jmin = wave_min(ls[0] == smin ? (double)lj[0] : inf);
        const bool win = ls[0] == smin && (double)lj[0] == jmin;
#pragma unroll
        for (int i = 0; i + 1 < NBC; ++i) {
            ls[i] = win ? ls[i + 1] : ls[i];
            lj[i] = win ? lj[i + 1] : lj[i];
        }
        ls[NBC - 1] = win ? inf : ls[NBC - 1];
        lj[NBC - 1] = win ? INT_MAX : lj[NBC - 1];
        if (live && lane == 0) {
            nbr[(size_t)b * c.nb + r] = (int)jmin;
            if (dist2) dist2[(size_t)b * c.nb + r] = smin;
        }
    }
}

// ---- the same selection on 3-D positions (cmpc_nbr_select3_dev): traj_all is n_total x (N+1) x 3 ----
//
// nbr_select_kernel with the third coordinate beside it.  The xy pairs keep the double2 tile; z gets a tile of
// its own, so a candidate and stage is still one 16-byte and one 8-byte LDS read, each over consecutive lanes:
// a b128 read is served 16 lanes at a time and a b64 read 32 lanes at a time, 256 contiguous bytes either way,
// one per bank.  The staging stores go stage-major down one candidate: consecutive threads are one row apart,
// kSelLd * 16 bytes = 4 dwords (mod 32 banks) in the xy tile, so the 8 lanes a b128 store serves at a time
// cover the 32 banks once, and kSelLdZ * 8 bytes = 2 dwords (mod 32) in the z tile, so the 16 lanes of a b64
// store do.  24 bytes per staged element: 16 x 129 x 24 B of tiles and the agents' own rows, 51 072 B per
// workgroup of 4 agents and 52 608 B of 8: 3 workgroups per compute unit.

constexpr int kSelLdZ = kSelTile + 1;  // padded row of the z tile (2 * kSelLdZ dwords = 2 mod 32)

template <int WAVES>
struct SelFetch3 {
    double2 v[sel_stage(WAVES)];
    double vz[sel_stage(WAVES)];
    double2 own;  // lane l: the wave's own agent at stage l of the chunk
    double ownz;
    int jj, kk;   // element 0 of this thread
};

template <int WAVES>
__device__ __forceinline__ void sel_fetch3(const NbrConst& c, const double* __restrict__ traj_all, int g, int lane,
                                           int j0, int kc0, int kc, int span, SelFetch3<WAVES>& f) {
    const size_t row = (size_t)(c.N + 1) * 3;
    f.jj = threadIdx.x / kc;
    f.kk = threadIdx.x - f.jj * kc;
    sel_walk<WAVES>(f.jj, f.kk, kc, span, [&](int e, int jj, int kk) {
        double2 v = {0.0, 0.0};  // past the population: never selected (j < n_total at the insertion)
        double vz = 0.0;
        if (j0 + jj < c.n_total) {
            const double* p = traj_all + (size_t)(j0 + jj) * row + (size_t)(kc0 + kk) * 3;
            v.x = p[0];
            v.y = p[1];
            vz = p[2];
        }
        f.v[e] = v;
        f.vz[e] = vz;
    });
    if (lane < kc) {
        const double* p = traj_all + (size_t)g * row + (size_t)(kc0 + lane) * 3;
        f.own = double2{p[0], p[1]};
        f.ownz = p[2];
    }
}

// sel_score with the third term: d = dx dx + dy dy + dz dz, summed left to right
template <bool FULL>
__device__ __forceinline__ void sel_score3(const double2 (*tile)[kSelLd], const double (*tilez)[kSelLdZ],
                                           const double2* own, const double* ownz, int lane, int kc,
                                           double (&run)[kSelPerLane], double (&sum)[kSelPerLane]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int kk = 0; kk < (FULL ? kSelChunk : kc); ++kk) {
        const double2 o = own[kk];
        const double oz = ownz[kk];
#pragma unroll
        for (int m = 0; m < kSelPerLane; ++m) {
            const double2 q = tile[kk][m * kWave + lane];
            const double qz = tilez[kk][m * kWave + lane];
            const double dx = q.x - o.x, dy = q.y - o.y, dz = qz - oz;
            const double d = dx * dx + dy * dy + dz * dz;
            run[m] = fmin(run[m], d);
            sum[m] = sum[m] + d;
        }
    }
}

template <int NBC, int WAVES>
__global__ __launch_bounds__(WAVES* kWave) void nbr_select3_kernel(NbrConst c, const double* __restrict__ traj_all,
                                                                   int* __restrict__ nbr, double* __restrict__ dist2) {
    __shared__ double2 tile[kSelChunk][kSelLd];
    __shared__ double tilez[kSelChunk][kSelLdZ];
    __shared__ double2 own[WAVES][kSelChunk];
    __shared__ double ownz[WAVES][kSelChunk];
    const int lane = threadIdx.x & (kWave - 1);
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int b = blockIdx.x * WAVES + w;
    const bool live = b < c.batch;  // wave-uniform; a wave past the batch still helps staging
    const int g = c.self_offset + (live ? b : c.batch - 1);
    const double inf = __builtin_inf();

    double ls[NBC];  // this lane's best candidates so far, ascending by (score, j)
    int lj[NBC];
#pragma unroll
    for (int i = 0; i < NBC; ++i) {
        ls[i] = inf;
        lj[i] = INT_MAX;
    }
    double run[kSelPerLane], sum[kSelPerLane];  // min and sum over the window's stages so far
#pragma unroll
    for (int m = 0; m < kSelPerLane; ++m) {
        run[m] = inf;
        sum[m] = 0.0;
    }

    // the steps of nbr_select_kernel: one tile per chunk of a long window, kSelChunk / W tiles side by side (rows
    // t * kc + kk of both tiles) for a window of W <= kSelChunk stages
    const int W = c.k1 - c.k0 + 1;
    const int nt = W <= kSelChunk ? kSelChunk / W : 1, span = nt * kSelTile;
    SelFetch3<WAVES> f;
    int j0 = 0, kc0 = c.k0;
    sel_fetch3(c, traj_all, g, lane, j0, kc0, min(kSelChunk, W), span, f);
    while (j0 < c.n_total) {
        const int kc = min(kSelChunk, c.k1 + 1 - kc0);
        __syncthreads();  // the previous step has been read
        sel_walk<WAVES>(f.jj, f.kk, kc, span, [&](int e, int jj, int kk) {
            tile[(jj / kSelTile) * kc + kk][jj % kSelTile] = f.v[e];
            tilez[(jj / kSelTile) * kc + kk][jj % kSelTile] = f.vz[e];
        });
        if (lane < kc) {
            own[w][lane] = f.own;
            ownz[w][lane] = f.ownz;
        }
        __syncthreads();
        const bool last = kc0 + kc > c.k1;  // the window's last chunk: the scores are complete
        const int nj0 = last ? j0 + span : j0, nkc0 = last ? c.k0 : kc0 + kc;
        if (nj0 < c.n_total) sel_fetch3(c, traj_all, g, lane, nj0, nkc0, min(kSelChunk, c.k1 + 1 - nkc0), span, f);
        for (int t = 0; t < nt && j0 + t * kSelTile < c.n_total; ++t) {
            if (kc == kSelChunk)
                sel_score3<true>(tile + t * kc, tilez + t * kc, own[w], ownz[w], lane, kc, run, sum);
            else
                sel_score3<false>(tile + t * kc, tilez + t * kc, own[w], ownz[w], lane, kc, run, sum);
            if (!last) continue;
#pragma unroll
            for (int m = 0; m < kSelPerLane; ++m) {
                const int j = j0 + t * kSelTile + m * kWave + lane;
                const double s = sum[m] != sum[m] ? inf : run[m];  // a NaN score counts as +inf
                run[m] = inf;
                sum[m] = 0.0;
                if (j < c.n_total && j != g && sel_less(s, j, ls[NBC - 1], lj[NBC - 1])) {
                    bool lt[NBC];
#pragma unroll
                    for (int i = 0; i < NBC; ++i) lt[i] = sel_less(s, j, ls[i], lj[i]);
#pragma unroll
                    for (int i = NBC - 1; i > 0; --i) {
                        ls[i] = lt[i - 1] ? ls[i - 1] : (lt[i] ? s : ls[i]);
                        lj[i] = lt[i - 1] ? lj[i - 1] : (lt[i] ? j : lj[i]);
                    }
                    ls[0] = lt[0] ? s : ls[0];
                    lj[0] = lt[0] ? j : lj[0];
                }
            }
        }
        j0 = nj0;
        kc0 = nkc0;
    }

    // the merge of nbr_select_kernel: nb times the wave's smallest list head by (score, j)
    for (int r = 0; r < c.nb; ++r) {
        const double smin = wave_min(ls[0]);
        const double jmin = wave_min(ls[0] == smin ? (double)lj[0] : inf);
        const bool win = ls[0] == smin && (double)lj[0] == jmin;
#pragma unroll
        for (int i = 0; i + 1 < NBC; ++i) {
            ls[i] = win ? ls[i + 1] : ls[i];
            lj[i] = win ? lj[i + 1] : lj[i];
        }
        ls[NBC - 1] = win ? inf : ls[NBC - 1];
        lj[NBC - 1] = win ? INT_MAX : lj[NBC - 1];
        if (live && lane == 0) {
            nbr[(size_t)b * c.nb + r] = (int)jmin;
            if (dist2) dist2[(size_t)b * c.nb + r] = smin;
        }
    }
}

}  // namespace

template <int WAVES>
static void sel_launch(const NbrConst& c, const double* traj_all, int* nbr, double* dist2, hipStream_t s) {
    const dim3 grid((c.batch + WAVES - 1) / WAVES), block(WAVES * kWave);
    // the per-lane list length is a compile-time size (registers): the smallest instantiation that holds nb
    if (c.nb <= 2)
        hipLaunchKernelGGL((nbr_select_kernel<2, WAVES>), grid, block, 0, s, c, traj_all, nbr, dist2);
    else if (c.nb <= 4)
        hipLaunchKernelGGL((nbr_select_kernel<4, WAVES>), grid, block, 0, s, c, traj_all, nbr, dist2);
    else
        hipLaunchKernelGGL((nbr_select_kernel<CMPC_MAX_MC - 4, WAVES>), grid, block, 0, s, c, traj_all, nbr, dist2);
}

hipError_t nbr_select_launch(const NbrConst& c, const double* traj_all, int* nbr, double* dist2, hipStream_t s) {
    if (c.batch == 0 || c.nb == 0) return hipSuccess;
    if (c.batch < kSelWideBatch)
        sel_launch<4>(c, traj_all, nbr, dist2, s);
    else
        sel_launch<8>(c, traj_all, nbr, dist2, s);
    return hipGetLastError();
}

template <int WAVES>
static void sel3_launch(const NbrConst& c, const double* traj_all, int* nbr, double* dist2, hipStream_t s) {
    const dim3 grid((c.batch + WAVES - 1) / WAVES), block(WAVES * kWave);
    if (c.nb <= 2)
        hipLaunchKernelGGL((nbr_select3_kernel<2, WAVES>), grid, block, 0, s, c, traj_all, nbr, dist2);
    else if (c.nb <= 4)
        hipLaunchKernelGGL((nbr_select3_kernel<4, WAVES>), grid, block, 0, s, c, traj_all, nbr, dist2);
    else
        hipLaunchKernelGGL((nbr_select3_kernel<CMPC_MAX_MC - 4, WAVES>), grid, block, 0, s, c, traj_all, nbr, dist2);
}

// the planar launch's rule for the agents per workgroup
hipError_t nbr_select3_launch(const NbrConst& c, const double* traj_all, int* nbr, double* dist2, hipStream_t s) {
    if (c.batch == 0 || c.nb == 0) return hipSuccess;
    if (c.batch < kSelWideBatch)
        sel3_launch<4>(c, traj_all, nbr, dist2, s);
    else
        sel3_launch<8>(c, traj_all, nbr, dist2, s);
    return hipGetLastError();
}

}  // namespace cmpc
