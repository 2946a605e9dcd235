// engine_host.h — host code shared by the four engine sources (engine.hip, unet_engine.hip, vae_engine.hip,
// linear_engine.hip): error reporting, grid sizes, environment switches, the tensor table, workspace carving, and the state,
// checks and entry-point bodies of the three stepped engines (UNET, var, Linear), and the data-parallel shard of the UNET and
// var engines (ShardSync, which the var engine hands on to its ConvAE trunk).  Internal C++ like trunk_api.h; not part of the
// C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cae_hip.h"

// engine.hip: sets the message cae_last_error() returns for the calling thread
void cae_detail_set_error(const char* msg);

namespace cae_internal {

// formats the message cae_last_error() returns and hands back `code`
inline int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    cae_detail_set_error(buf);
    return code;
}

#define HIP_TRY(expr)                                                                                                      \
    do {                                                                                                                   \
        hipError_t _e = (expr);                                                                                            \
        if (_e != hipSuccess)                                                                                              \
            return cae_internal::fail(CAE_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// workgroups of 256 threads for n elements: at least 1, at most cap (the grid-stride kernels walk the rest)
inline int blocks_for(long long n, int cap) { return (int)std::max(1ll, std::min((n + 255) / 256, (long long)cap)); }

// The tensor table: every named tensor of the model in the reference's state_dict order, with its offset in the parameter
// (arena 0) or buffer (arena 1) arena.  Tensors are 16-byte aligned.
struct TensorTable {
    std::vector<cae_tensor_info_t> tensors;
    int64_t n_param = 0, n_buf = 0;   // arena sizes (floats)

    // room for numel floats in an arena, no table entry
    int64_t reserve(int arena, int64_t numel) {
        int64_t& top = arena == 0 ? n_param : n_buf;
        top = (top + 3) & ~int64_t(3);
        const int64_t off = top;
        top += numel;
        return off;
    }
    // a table entry for a tensor at `offset`
    void list(const std::string& name, int arena, const std::vector<int64_t>& shape, int64_t offset) {
        cae_tensor_info_t t;
        memset(&t, 0, sizeof t);
        snprintf(t.name, sizeof t.name, "%s", name.c_str());
        t.arena = arena;
        t.ndim = (int)shape.size();
        t.numel = 1;
        for (size_t i = 0; i < shape.size(); i++) {
            t.shape[i] = shape[i];
            t.numel *= shape[i];
        }
        t.offset = offset;
        tensors.push_back(t);
    }
    int64_t add(const std::string& name, int arena, const std::vector<int64_t>& shape) {
        int64_t numel = 1;
        for (int64_t d : shape) numel *= d;
        const int64_t off = reserve(arena, numel);
        list(name, arena, shape, off);
        return off;
    }
    // both arenas end 16-byte aligned
    void close() {
        reserve(0, 0);
        reserve(1, 0);
    }
    int count() const { return (int)tensors.size(); }
    int info(int index, cae_tensor_info_t* out) const {
        if (!out || index < 0 || index >= count()) return fail(CAE_ERR_ARG, "tensor index out of range");
        *out = tensors[index];
        return CAE_OK;
    }
};

// Workspace regions laid end to end, each rounded up to `unit`: 256 for byte offsets (every region 256-byte aligned), 64 for
// the float offsets of a fp32 sub-arena
struct Carver {
    int64_t unit, top = 0;
    int64_t operator()(int64_t n) {
        const int64_t at = top;
        top += (n + unit - 1) / unit * unit;
        return at;
    }
};

// ---- the stepped engines: UNET, var, Linear ---------------------------------------------------------------------------
// One call per batch on the caller's stream; the losses of a batch land in a loss slot of the workspace.  `who` is the
// engine's C prefix ("unet", "vae", "lin"), used in messages.

constexpr int kStepLossSlots = 4096;   // (the ConvAE engine has its own count)

// A data-parallel rank's shard of a global batch (the *_forward_backward_sync / *_eval_step_sync entry points): rows
// [row0, row0 + batch) of global_batch rows, and the caller's fn (cae_hip.h) that sums a fp64 table over the ranks in place.
// world >= 1: the BatchNorm statistics are over the global batch (SyncBN); world 0: per rank.  The loss means are over the
// global batch either way.  A default-constructed value is the single-device step.
struct ShardSync {
    cae_allreduce_fn fn = nullptr;
    void* user = nullptr;
    int world = 0;
    int global_batch = 0;
    int row0 = 0;   // random masks / noise hash the rows' global indices

    bool sync_bn() const { return fn && world > 0; }   // BatchNorm sum tables go to fn too
    // rows behind the BatchNorm statistics and behind the loss means, for a local batch of B rows
    int stat_rows(int B) const { return sync_bn() ? global_batch : B; }
    int loss_rows(int B) const { return fn ? global_batch : B; }
};

// fn of a shard on a complete table of `count` doubles; a failing callback is an error of engine `who`
inline int call_allreduce(const ShardSync& s, const char* who, void* table, int64_t count) {
    if (s.fn(s.user, table, count) != 0)
        return fail(CAE_ERR_STATE, "%s: the all-reduce callback failed for a table of %lld doubles", who, (long long)count);
    return CAE_OK;
}

struct DataSet {
    const float* x = nullptr;
    const float* t = nullptr;   // target, or nullptr (scoring only)
    const float* m = nullptr;   // UNET: loss mask (N, mc, H, W), or nullptr
    int mc = 0;
    int64_t n = 0;
};

struct SteppedCore {
    char* ws = nullptr;
    hipStream_t stream = nullptr;
    int max_batch = 0;
    int64_t step = 0;         // completed optimiser steps
    int64_t ws_bytes = 0;
    int64_t off_losses = 0;   // kStepLossSlots x per_slot doubles
    int per_slot = 1;
    DataSet ds[2];
    ShardSync shard;          // the shard of the current *_sync call (ShardScope); a plain step leaves the default

    double* losses(int slot) const { return reinterpret_cast<double*>(ws + off_losses) + (size_t)per_slot * slot; }
};

// a *_sync call's shard, for the duration of the call
struct ShardScope {
    SteppedCore* c;
    ShardScope(SteppedCore* c_, const ShardSync& s) : c(c_) { c->shard = s; }
    ~ShardScope() { c->shard = ShardSync{}; }
};

// pointers_ok: the engine's arena pointers are all non-null
inline int bind_workspace(SteppedCore* c, const char* who, bool pointers_ok, void* ws, int64_t bytes) {
    if (!c || !pointers_ok || !ws) return fail(CAE_ERR_ARG, "%s_bind: null pointer", who);
    if (bytes < c->ws_bytes)
        return fail(CAE_ERR_ARG, "%s_bind: workspace of %lld bytes, need %lld", who, (long long)bytes, (long long)c->ws_bytes);
    if ((uintptr_t)ws & 255) return fail(CAE_ERR_ARG, "%s_bind: workspace must be 256-byte aligned", who);
    c->ws = static_cast<char*>(ws);
    return CAE_OK;
}

inline int set_stream(SteppedCore* c, const char* who, void* hip_stream) {
    if (!c) return fail(CAE_ERR_ARG, "%s_set_stream: null engine", who);
    c->stream = (hipStream_t)hip_stream;
    return CAE_OK;
}

inline int set_step(SteppedCore* c, const char* who, int64_t step) {
    if (!c || step < 0) return fail(CAE_ERR_ARG, "%s_set_step: bad argument", who);
    c->step = step;
    return CAE_OK;
}

inline int set_dataset(SteppedCore* c, const char* who, int which, const DataSet& d) {
    if (!c || which < 0 || which > 1 || !d.x || d.n < 1) return fail(CAE_ERR_ARG, "%s_set_dataset: bad argument", who);
    c->ds[which] = d;
    return CAE_OK;
}

// samples [start, start + batch) of data set `which` into loss slot `slot`
inline int check_batch(const SteppedCore* c, const char* who, int which, int64_t start, int batch, int slot, bool need_target) {
    if (!c || !c->ws) return fail(CAE_ERR_STATE, "%s: engine is not bound", who);
    if (which < 0 || which > 1 || !c->ds[which].x) return fail(CAE_ERR_STATE, "%s: data set %d is not set", who, which);
    if (need_target && !c->ds[which].t) return fail(CAE_ERR_STATE, "%s: data set %d has no target", who, which);
    if (batch < 1 || batch > c->max_batch) return fail(CAE_ERR_ARG, "%s: batch %d outside 1..%d", who, batch, c->max_batch);
    if (start < 0 || start + batch > c->ds[which].n)
        return fail(CAE_ERR_ARG, "%s: samples %lld..%lld outside the data set (%lld)", who, (long long)start,
                    (long long)(start + batch), (long long)c->ds[which].n);
    if (slot < 0 || slot >= kStepLossSlots)
        return fail(CAE_ERR_ARG, "%s: loss slot %d outside 0..%d", who, slot, kStepLossSlots - 1);
    return CAE_OK;
}

// check_batch for a shard (rows [row0, row0 + batch) of global_batch), which may be empty (batch 0: global batch < world, or
// the tail of a partial batch)
inline int check_shard(const SteppedCore* c, const char* who, int which, int64_t start, int batch, int row0, int global_batch,
                       int world, int slot, cae_allreduce_fn fn) {
    if (!fn || world < 0 || global_batch < 1 || batch < 0 || row0 < 0 || (int64_t)row0 + batch > global_batch)
        return fail(CAE_ERR_ARG, "%s: bad argument (batch %d at row %d of %d, world %d)", who, batch, row0, global_batch, world);
    if (batch > 0) return check_batch(c, who, which, start, batch, slot, true);
    if (!c->ws) return fail(CAE_ERR_STATE, "%s: engine is not bound", who);
    if (which < 0 || which > 1 || !c->ds[which].x || !c->ds[which].t) return fail(CAE_ERR_STATE, "%s: data set %d is not set", who, which);
    if (slot < 0 || slot >= kStepLossSlots) return fail(CAE_ERR_ARG, "%s: loss slot %d outside 0..%d", who, slot, kStepLossSlots - 1);
    return CAE_OK;
}

inline int check_score(const SteppedCore* c, const char* who, const float* x, int batch, const float* y) {
    if (!c || !c->ws) return fail(CAE_ERR_STATE, "%s_score: engine is not bound", who);
    if (!x || !y || batch < 1 || batch > c->max_batch) return fail(CAE_ERR_ARG, "%s_score: bad argument", who);
    return CAE_OK;
}

inline int read_losses(SteppedCore* c, const char* who, int first_slot, int count, double* out) {
    if (!c || !c->ws || !out || first_slot < 0 || count < 0 || first_slot + count > kStepLossSlots)
        return fail(CAE_ERR_ARG, "%s_read_losses: bad argument", who);
    HIP_TRY(hipMemcpyAsync(out, c->losses(first_slot), (size_t)count * c->per_slot * sizeof(double), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CAE_OK;
}

inline int sync(SteppedCore* c, const char* who) {
    if (!c) return fail(CAE_ERR_ARG, "%s_sync: null engine", who);
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CAE_OK;
}

}  // namespace cae_internal
