// host_residual.h - host only: the residual target over the interpolated input - cae_residual_scan, cae_residual_pack_rows,
// cae_residual_restore_f64 - over kernels_residual.h, with the items and size limits of host_baseline.h.  Included by
// stateless_host.h alone.
#pragma once

int64_t cae_residual_scan_workspace_bytes(int64_t n_case, int64_t h_out, int64_t w_out) {
    if (n_case < 1 || !baseline_sizes_ok(n_case, h_out, w_out)) return 0;
    return (n_case * baseline_items(h_out, w_out) + 1) * 3 * (int64_t)sizeof(double);      // the partials, then their fold
}

// the checks the three entry points share, on the ladder of the other stateless entry points; *a is filled when they pass
// and n_case > 0.  `other`: the fp32 operand beside low and the array written, both (n_case, h_out, w_out).
static int residual_args(const char* who, const CaseOperand& L, int64_t h_in, int64_t w_in, const float* other, const void* out,
                         int out_bytes, int64_t n_case, int64_t h_out, int64_t w_out, int mode, double rmin, double span, int enable,
                         RsArgs* a) {
    if (!known(L) || mode < CAE_INTERP_NEAREST || mode > CAE_INTERP_BICUBIC || h_in < 1 || h_in > BL_MAX_SIDE || w_in < 1 ||
        w_in > BL_MAX_SIDE || !baseline_sizes_ok(n_case, h_out, w_out))
        return fail(CAE_ERR_ARG, "%s: bad argument (a CAE_ELEM_* kind, a CAE_INTERP_* mode, n_case >= 0, sides of 1 to 2^30)", who);
    if (L.stride < 0) return fail(CAE_ERR_ARG, "%s: negative stride", who);
    if (n_case == 0) return CAE_OK;
    const int64_t plane_in = h_in * w_in, plane = h_out * w_out;
    const CaseOperand O{other, CAE_ELEM_F32, plane};
    if (!L.p || !other || !out) return fail(CAE_ERR_ARG, "%s: null pointer", who);
    if (any_shorter({{L, plane_in}})) return fail(CAE_ERR_ARG, "%s: a case stride is shorter than the plane", who);
    if (any_reaches(n_case, {{L, plane_in}, {O, plane}}))
        return fail(CAE_ERR_ARG, "%s: an operand reaches 2^60 elements from its pointer", who);
    if (any_misaligned({L, O}) || (uintptr_t)out % out_bytes != 0)
        return fail(CAE_ERR_ARG, "%s: pointers must be aligned to their element size", who);
    memset(a, 0, sizeof *a);
    a->low = (const unsigned char*)L.p, a->low_stride = L.stride, a->lk = L.kind;
    a->h_in = (int)h_in, a->w_in = (int)w_in, a->h_out = (int)h_out, a->w_out = (int)w_out;
    a->sy = (double)h_in / (double)h_out, a->sx = (double)w_in / (double)w_out;
    a->n_band = (int)((h_out + BL_ROWS - 1) / BL_ROWS), a->n_strip = (int)((w_out + BL_COLS - 1) / BL_COLS);
    a->items = n_case * baseline_items(h_out, w_out);
    a->in = other;
    a->rmin = rmin, a->span = span, a->enable = enable;
    return CAE_OK;
}

template <int OP>
static void residual_launch(const RsArgs& a, int mode, hipStream_t s) {
    const dim3 grid((unsigned)((a.items + 3) / 4));
    switch (mode) {
    case CAE_INTERP_NEAREST: hipLaunchKernelGGL((k_residual<0, OP>), grid, dim3(256), 0, s, a); break;
    case CAE_INTERP_BILINEAR: hipLaunchKernelGGL((k_residual<1, OP>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((k_residual<2, OP>), grid, dim3(256), 0, s, a); break;
    }
}

int cae_residual_scan(const void* low, int low_kind, int64_t low_stride, int64_t h_in, int64_t w_in, const float* target,
                      int64_t n_case, int64_t h_out, int64_t w_out, int mode, void* workspace, int64_t workspace_bytes,
                      void* hip_stream, double* out3) {
    if (!out3) return fail(CAE_ERR_ARG, "cae_residual_scan: null pointer");
    RsArgs a;
    if (int rc = residual_args("cae_residual_scan", CaseOperand{low, low_kind, low_stride}, h_in, w_in, target, out3, 1, n_case,
                               h_out, w_out, mode, 0.0, 0.0, 0, &a))
        return rc;
    out3[0] = 0.0, out3[1] = INFINITY, out3[2] = -INFINITY;
    if (n_case == 0) return CAE_OK;
    const int64_t need = cae_residual_scan_workspace_bytes(n_case, h_out, w_out);
    if (workspace_short(workspace, workspace_bytes, need)) return no_workspace("cae_residual_scan", need);
    hipStream_t s = (hipStream_t)hip_stream;
    a.part = (double*)workspace;
    double* folded = a.part + 3 * a.items;
    residual_launch<RS_SCAN>(a, mode, s);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_residual_fold, dim3(1), dim3(256), 0, s, (const double*)a.part, (long long)a.items, folded);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out3, folded, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return CAE_OK;
}

int cae_residual_pack_rows(const void* low, int low_kind, int64_t low_stride, int64_t h_in, int64_t w_in, const float* target,
                           int64_t n_case, int64_t h_out, int64_t w_out, int mode, double rmin, double span, int enable,
                           const int32_t* dst_row_dev, float* dst, void* hip_stream) {
    RsArgs a;
    if (int rc = residual_args("cae_residual_pack_rows", CaseOperand{low, low_kind, low_stride}, h_in, w_in, target, dst, 4,
                               n_case, h_out, w_out, mode, rmin, span, enable, &a))
        return rc;
    if (n_case == 0) return CAE_OK;
    if ((uintptr_t)dst_row_dev & 3) return fail(CAE_ERR_ARG, "cae_residual_pack_rows: pointers must be aligned to their element size");
    a.dst_rows = (const int*)dst_row_dev, a.y = dst;
    residual_launch<RS_PACK>(a, mode, (hipStream_t)hip_stream);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_residual_restore_f64(const void* low, int low_kind, int64_t low_stride, int64_t h_in, int64_t w_in, const float* y,
                             int64_t n_case, int64_t h_out, int64_t w_out, int mode, double rmin, double span, int enable,
                             double* out, void* hip_stream) {
    RsArgs a;
    if (int rc = residual_args("cae_residual_restore_f64", CaseOperand{low, low_kind, low_stride}, h_in, w_in, y, out, 8, n_case,
                               h_out, w_out, mode, rmin, span, enable, &a))
        return rc;
    if (n_case == 0) return CAE_OK;
    a.p = out;
    residual_launch<RS_RESTORE>(a, mode, (hipStream_t)hip_stream);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
