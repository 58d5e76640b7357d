// The C ABI's context object, the error helpers and the linear-model family's dimension rules shared by the
// host-side translation units (cmpc_api.hip, rounds_api.hip, round_log.hip).  Not part of the public header:
// cmpc.h keeps cmpc_ctx opaque.
#pragma once
#include <string>

#include <rccl/rccl.h>

#include "internal.h"

struct cmpc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;  // private stream for the host-pointer entry points
    char* ws = nullptr;            // device arena
    size_t ws_bytes = 0;
    char* order_ws = nullptr;      // scratch of cmpc_order_by_iters_dev (its own: the arena belongs to the solvers)
    size_t order_ws_bytes = 0;
    ncclComm_t comm = nullptr;     // RCCL communicator of cmpc_comm_init (multi-GPU exchange)
    int nranks = 1, rank = 0;      // of that communicator
    std::string err;
};

inline int fail(cmpc_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

inline int hip_fail(cmpc_ctx* c, hipError_t e, const char* where) {
    return fail(c, CMPC_ERR_DEVICE, std::string(where) + ": " + hipGetErrorString(e));
}

// the dimension rules of the linear-model family (cmpc_lin_*); no device call
inline int lin_const(cmpc_ctx* ctx, const cmpc_lin_params* prm, const cmpc_lin_dims* d, cmpc::LinConst* c) {
    if (!prm || !d) return fail(ctx, CMPC_ERR_ARG, "null argument");
    if (d->nx < 1 || d->nx > CMPC_MAX_NX || prm->ix < 0 || prm->ix >= d->nx || prm->iy < 0 || prm->iy >= d->nx ||
        prm->ix == prm->iy)
        return fail(ctx, CMPC_ERR_ARG, "bad linear-model dimensions (1 <= nx <= 12, position columns ix != iy in [0, nx))");
    if (d->N < 1 || d->nb < 0 || d->mo < 0 || d->mo + d->nb > CMPC_MAX_MC || d->batch < 0 || d->self_offset < 0)
        return fail(ctx, CMPC_ERR_ARG, "bad linear-model dimensions (N >= 1, mo + nb <= 16, batch >= 0, self_offset >= 0)");
    *c = cmpc::LinConst{d->N, d->nb, d->nx, d->mo, prm->ix, prm->iy, d->self_offset, -1, prm->min_dist, prm->wq};
    return CMPC_OK;
}

// ... and of its 3-D variant (cmpc_lin3_*): the planar rules, and a third position column apart from both
inline int lin_const(cmpc_ctx* ctx, const cmpc_lin3_params* prm, const cmpc_lin_dims* d, cmpc::LinConst* c) {
    if (!prm) return fail(ctx, CMPC_ERR_ARG, "null argument");
    const cmpc_lin_params planar{prm->ix, prm->iy, prm->min_dist, prm->wq};
    const int rc = lin_const(ctx, &planar, d, c);
    if (rc != CMPC_OK) return rc;
    if (prm->iz < 0 || prm->iz >= d->nx || prm->iz == prm->ix || prm->iz == prm->iy)
        return fail(ctx, CMPC_ERR_ARG, "bad linear-model dimensions (position columns ix, iy, iz pairwise different in [0, nx))");
    c->iz = prm->iz;
    return CMPC_OK;
}

#define HIP_TRY(expr)                                              \
    do {                                                           \
        hipError_t e_ = (expr);                                    \
        if (e_ != hipSuccess) return hip_fail(ctx, e_, #expr);     \
    } while (0)
