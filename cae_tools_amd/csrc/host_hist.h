// host_hist.h - host only: value distributions, the joint histogram of prediction against target: cae_joint_hist over
// kernels_hist.h.  Included by stateless_host.h alone.
#pragma once

static bool hist_sizes_ok(int64_t n_case, int64_t plane, int n_bin, int sub) {
    return n_case >= 0 && plane >= 0 && n_bin >= 1 && n_bin <= JH_MAX_BIN && sub >= 1 && sub <= JH_MAX_SUB &&
           (__int128)n_case * plane < ((__int128)1 << 40);
}

// the workgroups of a call, from (n_case, plane) alone: one per JH_WAVES items of cae_case_measures' cut, at most JH_MAX_GROUPS
static int64_t hist_groups(int64_t n_case, int64_t plane) { return ceil_capped(n_case * case_chunks(plane), JH_WAVES, JH_MAX_GROUPS); }

int64_t cae_joint_hist_workspace_bytes(int64_t n_case, int64_t plane, int n_bin, int sub) {
    if (n_case < 1 || plane < 1 || !hist_sizes_ok(n_case, plane, n_bin, sub)) return 0;
    return hist_groups(n_case, plane) * 2 * n_bin * 4 * (int64_t)sizeof(double);
}

int cae_joint_hist(const void* pred, int pred_kind, int64_t pred_stride, const void* actual, int actual_kind,
                   int64_t actual_stride, int64_t n_case, int64_t plane, double lo, double hi, int n_bin, int sub,
                   int64_t* joint, int64_t* marg, double* cond, int64_t* outside, void* workspace, int64_t workspace_bytes,
                   void* hip_stream) {
    const CaseOperand P{pred, pred_kind, pred_stride}, A{actual, actual_kind, actual_stride};
    if (!known(P) || !known(A) || !hist_sizes_ok(n_case, plane, n_bin, sub))
        return fail(CAE_ERR_ARG, "cae_joint_hist: bad argument (CAE_ELEM_* kinds, n_case >= 0, plane >= 0, 1 <= n_bin <= %d, "
                                 "1 <= sub <= %d, n_case * plane < 2^40)", JH_MAX_BIN, JH_MAX_SUB);
    const int n_fine = n_bin * sub;
    const double scale = (double)n_fine / (hi - lo);
    if (!is_finite(lo) || !is_finite(hi) || !(hi > lo) || !is_finite(scale) || !(scale > 0.0))
        return fail(CAE_ERR_ARG, "cae_joint_hist: lo and hi must be finite, hi > lo, and n_bin * sub / (hi - lo) finite and not zero");
    if (P.stride < 0 || A.stride < 0) return fail(CAE_ERR_ARG, "cae_joint_hist: negative stride");
    if (((uintptr_t)joint & 7) || ((uintptr_t)marg & 7) || ((uintptr_t)cond & 7) || ((uintptr_t)outside & 7))
        return fail(CAE_ERR_ARG, "cae_joint_hist: the outputs must be 8-byte aligned");
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t joint_bytes = (size_t)n_bin * n_bin * sizeof(int64_t), marg_bytes = (size_t)2 * n_fine * sizeof(int64_t),
                 cond_bytes = (size_t)2 * n_bin * 4 * sizeof(double), outside_bytes = 4 * sizeof(int64_t);
    if (n_case == 0 || plane == 0) {        // no pixel, no pair: the outputs that are given are zeroed, no operand is looked at
        if (joint) HIP_TRY(hipMemsetAsync(joint, 0, joint_bytes, s));
        if (marg) HIP_TRY(hipMemsetAsync(marg, 0, marg_bytes, s));
        if (cond) HIP_TRY(hipMemsetAsync(cond, 0, cond_bytes, s));
        if (outside) HIP_TRY(hipMemsetAsync(outside, 0, outside_bytes, s));
        return CAE_OK;
    }
    if (!P.p || !A.p || !joint || !marg || !cond || !outside) return fail(CAE_ERR_ARG, "cae_joint_hist: null pointer");
    if (any_shorter({{P, plane}, {A, plane}})) return fail(CAE_ERR_ARG, "cae_joint_hist: a case stride is shorter than the plane");
    if (any_reaches(n_case, {{P, plane}, {A, plane}}))
        return fail(CAE_ERR_ARG, "cae_joint_hist: an operand reaches 2^60 elements from its pointer");
    if (any_misaligned({P, A})) return fail(CAE_ERR_ARG, "cae_joint_hist: pointers must be aligned to their element size");
    const int64_t need = cae_joint_hist_workspace_bytes(n_case, plane, n_bin, sub);
    if (workspace_short(workspace, workspace_bytes, need)) return no_workspace("cae_joint_hist", need);
    const int64_t n_group = hist_groups(n_case, plane);
    const int per = 2 * n_bin * 4;
    JhArgs a;
    memset(&a, 0, sizeof a);
    a.p = (const unsigned char*)P.p, a.a = (const unsigned char*)A.p;
    a.p_stride = P.stride, a.a_stride = A.stride, a.plane = plane;
    a.nch = (int)case_chunks(plane), a.items = n_case * case_chunks(plane);
    a.lo = lo, a.hi = hi, a.scale = scale;
    a.n_bin = n_bin, a.sub = sub, a.n_fine = n_fine;
    a.magic = (unsigned)(((1u << JH_SHIFT) + sub - 1) / sub);
    a.joint = (unsigned long long*)joint, a.marg = (unsigned long long*)marg, a.outside = (unsigned long long*)outside;
    a.part = (double*)workspace;
    HIP_TRY(hipMemsetAsync(joint, 0, joint_bytes, s));
    HIP_TRY(hipMemsetAsync(marg, 0, marg_bytes, s));
    HIP_TRY(hipMemsetAsync(outside, 0, outside_bytes, s));
    const size_t lds = (size_t)JH_WAVES * per * sizeof(double) + ((size_t)n_bin * n_bin + 2 * (size_t)n_fine) * sizeof(unsigned);
    const dim3 grid((unsigned)n_group);
    with_kinds(P.kind, A.kind, [&](auto KP, auto KA) {
        launch_with_lds<k_joint_hist<decltype(KP)::value, decltype(KA)::value>>(grid, dim3(64 * JH_WAVES), lds, s, a);
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_joint_hist_fold<JH_WAVES>), dim3((unsigned)((per + 255) / 256)), dim3(256), 0, s, (const double*)workspace,
                       (int)n_group, per, cond);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
