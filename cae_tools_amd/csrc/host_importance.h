// host_importance.h - host only: permutation importance, a batch with rows drawn from other cases and the comparison of its scores:
// cae_normalise_pack_gather and cae_case_importance over kernels_importance.h.  Included by stateless_host.h alone.
#pragma once

int cae_normalise_pack_gather(const float* src, int64_t n_src, int c_src, int64_t hw, float* dst, int64_t n_dst, int c_dst, int c_off,
                              float vmin, float range, int enable, const int32_t* row_dev, void* hip_stream) {
    if (n_src < 0 || n_dst < 0 || c_src < 1 || hw < 0 || c_off < 0 || c_off > c_dst - c_src)
        return fail(CAE_ERR_ARG, "cae_normalise_pack_gather: bad argument (n_src >= 0, n_dst >= 0, c_src >= 1, hw >= 0, "
                                 "0 <= c_off <= c_dst - c_src)");
    if (n_src > 0x7fffffffLL || n_dst > 0x7fffffffLL) return fail(CAE_ERR_ARG, "cae_normalise_pack_gather: more than 2^31 - 1 rows");
    if (n_dst == 0 || hw == 0) return CAE_OK;
    if ((!src && n_src > 0) || !dst || !row_dev) return fail(CAE_ERR_ARG, "cae_normalise_pack_gather: null pointer");
    if ((__int128)n_src * c_src * hw > ((__int128)1 << 60) || (__int128)n_dst * c_dst * hw > ((__int128)1 << 60))
        return fail(CAE_ERR_ARG, "cae_normalise_pack_gather: an operand reaches 2^60 elements from its pointer");
    if (((uintptr_t)src & 3) || ((uintptr_t)dst & 3) || ((uintptr_t)row_dev & 3))
        return fail(CAE_ERR_ARG, "cae_normalise_pack_gather: pointers must be 4-byte aligned");
    const long long total = (long long)n_dst * c_src * hw;
    const int blocks = (int)ceil_capped(total, 256 * 8, 8192);
    hipLaunchKernelGGL((k_normalise_pack_gather<256>), dim3(blocks), dim3(256), 0, (hipStream_t)hip_stream, src, (long long)n_src, total,
                       c_src, (long long)hw, dst, c_dst, c_off, vmin, range, enable, (const int*)row_dev);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

static int64_t importance_tiles(int64_t plane) { return (plane + IM_TILE - 1) / IM_TILE; }

int64_t cae_case_importance_workspace_bytes(int64_t n_case, int64_t plane) {
    if (n_case < 1 || plane < 1 || (__int128)n_case * plane > ((__int128)1 << 60)) return 0;
    return n_case * importance_tiles(plane) * IM_SUMS * (int64_t)sizeof(double);
}

int cae_case_importance(const float* base, int64_t base_stride, const float* pert, int64_t pert_stride, const void* actual,
                        int actual_kind, int64_t actual_stride, int64_t n_case, int64_t plane, double vmin, double range,
                        double* sums, double* map, void* workspace, int64_t workspace_bytes, void* hip_stream) {
    const CaseOperand B{base, CAE_ELEM_F32, base_stride}, Q{pert, CAE_ELEM_F32, pert_stride}, A{actual, actual_kind, actual_stride};
    if (!known(A) || n_case < 0 || plane < 0)
        return fail(CAE_ERR_ARG, "cae_case_importance: bad argument (a CAE_ELEM_* kind, n_case >= 0, plane >= 0)");
    if (B.stride < 0 || Q.stride < 0 || A.stride < 0) return fail(CAE_ERR_ARG, "cae_case_importance: negative stride");
    if (!is_finite(vmin) || !is_finite(range)) return fail(CAE_ERR_ARG, "cae_case_importance: vmin and range must be finite");
    if (n_case == 0 || plane == 0) return CAE_OK;
    if (!B.p || !Q.p || !A.p || !sums) return fail(CAE_ERR_ARG, "cae_case_importance: null pointer");
    if (any_shorter({{B, plane}, {Q, plane}, {A, plane}}))
        return fail(CAE_ERR_ARG, "cae_case_importance: a case stride is shorter than the plane");
    if (any_reaches(n_case, {{B, plane}, {Q, plane}, {A, plane}}) || (__int128)n_case * plane > ((__int128)1 << 60))
        return fail(CAE_ERR_ARG, "cae_case_importance: an operand reaches 2^60 elements from its pointer");
    if (any_misaligned({B, Q, A}) || ((uintptr_t)sums & 7) || ((uintptr_t)map & 7) || ((uintptr_t)workspace & 15))
        return fail(CAE_ERR_ARG, "cae_case_importance: pointers must be aligned to their element size, the workspace to 16 bytes");
    const int64_t need = cae_case_importance_workspace_bytes(n_case, plane);
    if (!workspace || workspace_bytes < need) return no_workspace("cae_case_importance", need);
    hipStream_t s = (hipStream_t)hip_stream;
    ImArgs a;
    memset(&a, 0, sizeof a);
    a.base = base, a.pert = pert, a.a = (const unsigned char*)actual;
    a.base_stride = base_stride, a.pert_stride = pert_stride, a.a_stride = actual_stride;
    a.n_case = n_case, a.plane = plane, a.n_tile = importance_tiles(plane);
    a.items = map ? a.n_tile : a.n_tile * ((n_case + IM_RUN - 1) / IM_RUN);
    a.vmin = vmin, a.range = range, a.part = (double*)workspace, a.map = map;
    const dim3 grid((unsigned)ceil_capped(a.items, IM_WAVES, map ? (int64_t)1 << 20 : 16384));
    with_kind(A.kind, [&](auto KA) {
        if (map) hipLaunchKernelGGL((k_case_importance<decltype(KA)::value, true>), grid, dim3(64 * IM_WAVES), 0, s, a);
        else hipLaunchKernelGGL((k_case_importance<decltype(KA)::value, false>), grid, dim3(64 * IM_WAVES), 0, s, a);
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_importance_fold<IM_WAVES>), dim3((unsigned)ceil_capped(n_case, IM_WAVES, 8192)), dim3(64 * IM_WAVES), 0, s,
                       (const double*)workspace, (long long)n_case, (long long)a.n_tile, sums);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
