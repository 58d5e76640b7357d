// A round's experiment-log rows on the device (include/cmpc.h, cmpc_round_log_dev): what the reference appends
// per control step to states.dat / u.dat / plan_dist.dat (config/base_class.py:64-99) —
//   state[b, :] = xPred[0] = z[b, 0 .. nx),  u[b, :] = uPred[0] = z[b, (nx+ns)(N+1) .. +nu),
//   look_ahead[b] = xPred[-1, look_col] - xPred[0, look_col] = z[b, (nx+ns) N + look_col] - z[b, look_col]
// — and copies of the round's kkt / iters / status, so a host that queues 100 rounds reads the run once.
// Pure data movement: one thread per output element, the destinations laid end to end over the grid
// (state | u | look_ahead | kkt | iters | status, a null one taking no threads), so consecutive threads write
// consecutive addresses of a destination.  Values are copied as they are (a NaN z gives NaN rows); the
// look-ahead is one subtraction.
#include <climits>

#include "ctx.h"

namespace cmpc {

namespace {

constexpr int kLogBlock = 256;

__global__ __launch_bounds__(kLogBlock) void round_log_kernel(LogConst c, LogPtrs p) {
    size_t i = (size_t)blockIdx.x * kLogBlock + threadIdx.x;
    const size_t B = (size_t)c.batch;
    size_t n = p.state ? B * c.nx : 0;
    if (i < n) {
        const size_t b = i / c.nx;
        p.state[i] = p.z[b * c.nz + (i - b * c.nx)];
        return;
    }
    i -= n;
    n = p.u ? B * c.nu : 0;
    if (i < n) {
        const size_t b = i / c.nu;
        p.u[i] = p.z[b * c.nz + c.u_off + (i - b * c.nu)];
        return;
    }
    i -= n;
    n = p.look ? B : 0;
    if (i < n) {
        p.look[i] = p.z[i * c.nz + c.hi] - p.z[i * c.nz + c.lo];
        return;
    }
    i -= n;
    n = p.kkt_out ? B : 0;
    if (i < n) {
        p.kkt_out[i] = p.kkt[i];
        return;
    }
    i -= n;
    n = p.iters_out ? B : 0;
    if (i < n) {
        p.iters_out[i] = p.iters[i];
        return;
    }
    i -= n;
    if (p.status_out && i < B) p.status_out[i] = p.status[i];
}

}  // namespace

hipError_t round_log_launch(const LogConst& c, const LogPtrs& p, hipStream_t s) {
    if (c.batch <= 0) return hipSuccess;
    const size_t per = (p.state ? c.nx : 0) + (p.u ? c.nu : 0) + (p.look ? 1 : 0) + (p.kkt_out ? 1 : 0) +
                       (p.iters_out ? 1 : 0) + (p.status_out ? 1 : 0);
    const size_t total = per * (size_t)c.batch;
    if (total == 0) return hipSuccess;
    const dim3 grid((unsigned)((total + kLogBlock - 1) / kLogBlock)), block(kLogBlock);
    hipLaunchKernelGGL(round_log_kernel, grid, block, 0, s, c, p);
    return hipGetLastError();
}

}  // namespace cmpc

extern "C" int cmpc_round_log_dev(cmpc_ctx* ctx, const cmpc_log_dims* d, const double* z, const double* kkt,
                                  const int* iters, const int* status, const cmpc_log_row* row, void* stream) {
    if (!ctx) return CMPC_ERR_ARG;
    if (!d || !z || !row) return fail(ctx, CMPC_ERR_ARG, "null argument");
    if (d->batch < 0 || d->N < 1 || d->nx < 1 || d->nx > CMPC_MAX_NX || d->nu < 1 || d->nu > CMPC_MAX_NU || d->ns < 0 ||
        d->ns > CMPC_MAX_NS)
        return fail(ctx, CMPC_ERR_ARG, "bad log dimensions (batch >= 0, N >= 1, 1 <= nx <= 12, 1 <= nu <= 4, 0 <= ns <= 4)");
    if (d->look_col < 0 || d->look_col >= d->nx) return fail(ctx, CMPC_ERR_ARG, "look_col outside [0, nx)");
    if ((row->kkt && !kkt) || (row->iters && !iters) || (row->status && !status))
        return fail(ctx, CMPC_ERR_ARG, "a log destination of kkt / iters / status without its source");
    if (d->batch == 0) return CMPC_OK;
    const long long nxe = d->nx + d->ns, nz = nxe * (d->N + 1) + 2LL * d->nu * d->N;
    if (nz > INT_MAX) return fail(ctx, CMPC_ERR_ARG, "horizon too long");
    HIP_TRY(hipSetDevice(ctx->device));
    const cmpc::LogConst c{d->batch, d->nx, d->nu, (int)nz, (int)(nxe * (d->N + 1)), (int)(nxe * d->N + d->look_col),
                           d->look_col};
    const cmpc::LogPtrs p{z, kkt, iters, status, row->state, row->u, row->look_ahead, row->kkt, row->iters, row->status};
    HIP_TRY(cmpc::round_log_launch(c, p, (hipStream_t)stream));
    return CMPC_OK;
}
