// host_ssim.h - host only: structural similarity of prediction against target, cae_case_ssim, over kernels_ssim.h.
// Included by stateless_host.h alone.
#pragma once

// the side of the next scale: 2 x 2 pooling with padding size mod 2 on both sides
static int64_t ssim_pooled(int64_t side) { return (side + 2 * (side & 1)) / 2; }

// the scales' shapes and the cut of each into (band, strip) items, from (h, w) alone; returns the items of one case
static int64_t ssim_plan(int64_t h, int64_t w, int n_scale, SsScale* sc, int64_t* plane_doubles) {
    int64_t per_case = 0, planes = 0;
    for (int s = 0; s < n_scale; s++) {
        sc[s].h = (int)h, sc[s].w = (int)w;
        sc[s].rb = ss_band_rows((int)h);
        const bool any = h >= SS_WIN && w >= SS_WIN;
        sc[s].n_band = any ? (int)((h - SS_HALO + sc[s].rb - 1) / sc[s].rb) : 0;
        sc[s].n_strip = any ? (int)((w - SS_HALO + SS_COLS - 1) / SS_COLS) : 0;
        per_case += (int64_t)sc[s].n_band * sc[s].n_strip;
        if (s > 0) planes += 2 * h * w;
        h = ssim_pooled(h), w = ssim_pooled(w);
    }
    if (plane_doubles) *plane_doubles = planes;
    return per_case;
}

static bool ssim_sizes_ok(int64_t n_case, int64_t h, int64_t w, int n_scale) {
    if (n_case < 0 || h < 1 || h > SS_MAX_SIDE || w < 1 || w > SS_MAX_SIDE || n_scale < 1 || n_scale > SS_SCALES) return false;
    SsScale sc[SS_SCALES];
    int64_t planes = 0;
    const int64_t per_case = ssim_plan(h, w, n_scale, sc, &planes);
    return (__int128)n_case * per_case <= 0x7fffffffLL && (__int128)n_case * planes < ((__int128)1 << 56);
}

int64_t cae_case_ssim_workspace_bytes(int64_t n_case, int64_t h, int64_t w, int n_scale) {
    if (n_case < 1 || !ssim_sizes_ok(n_case, h, w, n_scale)) return 0;
    SsScale sc[SS_SCALES];
    int64_t planes = 0;
    const int64_t per_case = ssim_plan(h, w, n_scale, sc, &planes);
    return n_case * (planes + 3 * per_case) * (int64_t)sizeof(double);
}

int cae_case_ssim(const void* pred, int pred_kind, int64_t pred_stride, const void* actual, int actual_kind,
                  int64_t actual_stride, int64_t n_case, int64_t h, int64_t w, int n_scale, double shift, double scale,
                  const double* window, double* sums, void* workspace, int64_t workspace_bytes, void* hip_stream) {
    const CaseOperand P{pred, pred_kind, pred_stride}, A{actual, actual_kind, actual_stride};
    if (!known(P) || !known(A) || !ssim_sizes_ok(n_case, h, w, n_scale))
        return fail(CAE_ERR_ARG, "cae_case_ssim: bad argument (CAE_ELEM_* kinds, n_case >= 0, 1 <= h, w <= %d, 1 <= n_scale <= %d)",
                    SS_MAX_SIDE, SS_SCALES);
    if (!is_finite(shift) || !is_finite(scale)) return fail(CAE_ERR_ARG, "cae_case_ssim: shift and scale must be finite");
    if (n_case == 0) return CAE_OK;
    const int64_t plane = h * w;
    if (!P.p || !A.p || !window || !sums) return fail(CAE_ERR_ARG, "cae_case_ssim: null pointer");
    if (any_shorter({{P, plane}, {A, plane}})) return fail(CAE_ERR_ARG, "cae_case_ssim: a case stride is shorter than the plane");
    if (any_reaches(n_case, {{P, plane}, {A, plane}}))
        return fail(CAE_ERR_ARG, "cae_case_ssim: an operand reaches 2^60 elements from its pointer");
    if (any_misaligned({P, A}) || ((uintptr_t)sums & 7) || ((uintptr_t)workspace & 7))
        return fail(CAE_ERR_ARG, "cae_case_ssim: pointers must be aligned to their element size, the workspace to 8 bytes");
    const int64_t need = cae_case_ssim_workspace_bytes(n_case, h, w, n_scale);
    if (need > 0 && (!workspace || workspace_bytes < need)) return no_workspace("cae_case_ssim", need);
    hipStream_t s = (hipStream_t)hip_stream;
    SsArgs a;
    memset(&a, 0, sizeof a);
    int64_t planes = 0;
    const int64_t per_case = ssim_plan(h, w, n_scale, a.s, &planes);
    a.n_scale = n_scale, a.n_case = n_case, a.items = n_case * per_case;
    a.shift = shift, a.scale = scale;
    for (int t = 0; t < SS_WIN; t++) a.win.g[t] = window[t];
    double* ws = (double*)workspace;
    a.part = ws + n_case * planes;
    a.s[0].x = (const unsigned char*)pred, a.s[0].y = (const unsigned char*)actual;
    a.s[0].x_stride = pred_stride, a.s[0].y_stride = actual_stride, a.s[0].xk = pred_kind, a.s[0].yk = actual_kind;
    int64_t first = 0;
    for (int k = 0; k < n_scale; k++) {
        SsScale& c = a.s[k];
        c.first = first;
        first += n_case * c.n_band * c.n_strip;
        if (k + 1 == n_scale) break;
        // the planes of scale k + 1: [case][x | y][h][w] doubles, pooled from scale k
        SsScale& d = a.s[k + 1];
        const int64_t per = (int64_t)d.h * d.w;
        d.x = (const unsigned char*)ws, d.y = (const unsigned char*)(ws + per);
        d.x_stride = d.y_stride = 2 * per, d.xk = d.yk = CAE_ELEM_F64;
        hipLaunchKernelGGL(k_ssim_pool, dim3((unsigned)ceil_capped(n_case * per, 256, 65536)), dim3(256), 0, s, c.x, c.xk,
                           (long long)c.x_stride, c.y, c.yk, (long long)c.y_stride, (long long)n_case, c.h, c.w,
                           k == 0 ? shift : 0.0, k == 0 ? scale : 1.0, ws);
        HIP_TRY(hipGetLastError());
        ws += n_case * 2 * per;
    }
    if (a.items > 0) {
        hipLaunchKernelGGL(k_case_ssim, dim3((unsigned)((a.items + 3) / 4)), dim3(256), 0, s, a);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_ssim_fold, dim3((unsigned)ceil_capped(n_case * n_scale * 3, 256, 4096)), dim3(256), 0, s, a, sums);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
