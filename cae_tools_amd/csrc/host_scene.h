// host_scene.h - host only: a box model applied to a whole scene, tiles out and the blended scene back: cae_scene_gather and
// cae_scene_blend over kernels_scene.h.  Included by stateless_host.h alone.
#pragma once

// tiles along an axis of `extent` pixels for a box side and an overlap: 1 + ceil((extent - box) / (box - overlap))
static int64_t scene_tiles_along(int64_t extent, int box, int overlap) {
    const int64_t s = box - overlap;
    return 1 + (extent - box + s - 1) / s;
}

static int scene_geom_check(const char* who, const cae_scene_geom* g, bool with_scale) {
    if (!g) return fail(CAE_ERR_ARG, "%s: null geometry", who);
    if (g->h < 1 || g->w < 1 || g->Y < g->h || g->X < g->w || g->Y > ((int64_t)1 << 30) || g->X > ((int64_t)1 << 30))
        return fail(CAE_ERR_ARG, "%s: a scene of %lld x %lld pixels does not hold a box of %d x %d (sides up to 2^30)", who,
                    (long long)g->Y, (long long)g->X, g->h, g->w);
    if (g->oy < 0 || g->oy >= g->h || g->ox < 0 || g->ox >= g->w)
        return fail(CAE_ERR_ARG, "%s: the overlap (%d, %d) must be at least 0 and below the box (%d, %d)", who, g->oy, g->ox, g->h, g->w);
    if (with_scale) {
        if (g->sy < 1 || g->sx < 1) return fail(CAE_ERR_ARG, "%s: the scale (%d, %d) must be at least 1", who, g->sy, g->sx);
        if ((__int128)4 * g->h * g->sy * g->w * g->sx >= ((__int128)1 << 29))
            return fail(CAE_ERR_ARG, "%s: 4 H W must stay below 2^29 (the weights times an fp32 value are then exact in fp64)", who);
    }
    return CAE_OK;
}

int cae_scene_gather(const cae_scene_geom* geom, const void* src, int src_kind, int64_t n_t, int c_src, int64_t t0,
                     int64_t n_t_call, int64_t ky0, int64_t n_ky, float* dst, int c_dst, int c_off, float vmin, float range,
                     int enable, int32_t* invalid, void* hip_stream) {
    if (const int rc = scene_geom_check("cae_scene_gather", geom, false)) return rc;
    if (!kind_known(src_kind) || n_t < 0 || c_src < 1 || c_off < 0 || c_off > c_dst - c_src ||
        t0 < 0 || n_t_call < 0 || t0 > n_t - n_t_call || ky0 < 0 || n_ky < 0)
        return fail(CAE_ERR_ARG, "cae_scene_gather: bad argument (a CAE_ELEM_* kind, the time range inside the variable, the channels inside the batch)");
    const int64_t n_y = scene_tiles_along(geom->Y, geom->h, geom->oy), n_x = scene_tiles_along(geom->X, geom->w, geom->ox);
    if (ky0 > n_y - n_ky) return fail(CAE_ERR_ARG, "cae_scene_gather: tile rows %lld .. %lld of %lld", (long long)ky0,
                                      (long long)(ky0 + n_ky), (long long)n_y);
    if (n_t_call == 0 || n_ky == 0) return CAE_OK;
    if (!src || !dst || !invalid) return fail(CAE_ERR_ARG, "cae_scene_gather: null pointer");
    if (((uintptr_t)src % elem_bytes(src_kind)) || ((uintptr_t)dst & 3) || ((uintptr_t)invalid & 3))
        return fail(CAE_ERR_ARG, "cae_scene_gather: pointers must be aligned to their element size");
    const __int128 per = (__int128)c_src * geom->h * geom->w, tiles = (__int128)n_t_call * n_ky * n_x;
    if (per > 0x7fffffffLL || (__int128)c_dst * geom->h * geom->w > 0x7fffffffLL || tiles > 0x7fffffffLL ||
        tiles * c_dst * geom->h * geom->w > ((__int128)1 << 60) || (__int128)n_t * c_src * geom->Y * geom->X > ((__int128)1 << 60))
        return fail(CAE_ERR_ARG, "cae_scene_gather: too large (2^31 - 1 tiles and box elements, 2^60 elements per operand)");
    SgArgs a;
    memset(&a, 0, sizeof a);
    a.src = (const unsigned char*)src, a.Y = geom->Y, a.X = geom->X, a.c_src = c_src, a.h = geom->h, a.w = geom->w;
    a.stride_y = geom->h - geom->oy, a.stride_x = geom->w - geom->ox, a.n_x = n_x;
    a.t0 = t0, a.ky0 = ky0, a.n_ky = n_ky, a.total = (long long)(tiles * per);
    a.dst = dst, a.c_dst = c_dst, a.c_off = c_off, a.vmin = vmin, a.range = range, a.enable = enable, a.invalid = (int*)invalid;
    const dim3 grid((unsigned)ceil_capped(a.total, 256 * 4, 8192));
    hipStream_t s = (hipStream_t)hip_stream;
    with_kind(src_kind, [&](auto KS) { hipLaunchKernelGGL((k_scene_gather<decltype(KS)::value>), grid, dim3(256), 0, s, a); });
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_scene_blend(const cae_scene_geom* geom, const float* pred, const int32_t* invalid, int64_t k0, int64_t n_k,
                    const float* carry_pred, const int32_t* carry_invalid, int64_t carry_k0, int64_t carry_n_k,
                    int64_t n_t_call, int c_out, int64_t row0, int64_t row1, double vmin, double range, double* out,
                    int64_t out_t_stride, int64_t* nan_pixels, void* hip_stream) {
    if (const int rc = scene_geom_check("cae_scene_blend", geom, true)) return rc;
    const int64_t n_y = scene_tiles_along(geom->Y, geom->h, geom->oy), n_x = scene_tiles_along(geom->X, geom->w, geom->ox);
    const int64_t H = (int64_t)geom->h * geom->sy, W = (int64_t)geom->w * geom->sx;
    const int64_t Ys = geom->Y * geom->sy, Xs = geom->X * geom->sx;
    if (Ys > ((int64_t)1 << 30) || Xs > ((int64_t)1 << 30))
        return fail(CAE_ERR_ARG, "cae_scene_blend: an output of %lld x %lld pixels (sides up to 2^30)", (long long)Ys, (long long)Xs);
    if (n_t_call < 0 || c_out < 1 || k0 < 0 || n_k < 0 || k0 > n_y - n_k || carry_n_k < 0 || carry_k0 < 0 || carry_k0 > n_y - carry_n_k ||
        row0 < 0 || row1 < row0 || row1 > Ys || out_t_stride < 0 || (n_t_call > 1 && out_t_stride < (__int128)c_out * Ys * Xs))
        return fail(CAE_ERR_ARG, "cae_scene_blend: bad argument (tile rows inside the scene's %lld, output rows inside its %lld, "
                                 "a time stride of at least a scene)", (long long)n_y, (long long)Ys);
    if (carry_n_k > 0 && carry_k0 + carry_n_k > k0)
        return fail(CAE_ERR_ARG, "cae_scene_blend: the carried tile rows must come before the new ones");
    if (n_t_call == 0 || row1 == row0) return CAE_OK;
    if (n_t_call * c_out > 65535) return fail(CAE_ERR_ARG, "cae_scene_blend: more than 65535 (time step, channel) planes in a call");
    if (!pred || !invalid || !out || !nan_pixels || (carry_n_k > 0 && (!carry_pred || !carry_invalid)))
        return fail(CAE_ERR_ARG, "cae_scene_blend: null pointer");
    if (((uintptr_t)pred & 3) || ((uintptr_t)invalid & 3) || ((uintptr_t)carry_pred & 3) || ((uintptr_t)carry_invalid & 3) ||
        ((uintptr_t)out & 7) || ((uintptr_t)nan_pixels & 7))
        return fail(CAE_ERR_ARG, "cae_scene_blend: pointers must be aligned to their element size");
    const __int128 limit = (__int128)1 << 60;
    if ((__int128)n_t_call * (n_k > carry_n_k ? n_k : carry_n_k) * n_x * c_out * H * W > limit ||
        (__int128)(n_t_call - 1) * out_t_stride + (__int128)c_out * Ys * Xs > limit)
        return fail(CAE_ERR_ARG, "cae_scene_blend: an operand reaches 2^60 elements from its pointer");
    // every tile row that covers an output row of the call must be in one of the two runs
    const int64_t SY = (int64_t)(geom->h - geom->oy) * geom->sy, LY = (geom->Y - geom->h) * geom->sy;
    auto origin = [&](int64_t k) { return k * SY < LY ? k * SY : LY; };
    for (int64_t k = 0; k < n_y; k++) {
        if (origin(k) + H <= row0 || origin(k) >= row1) continue;
        const bool here = (k >= k0 && k < k0 + n_k) || (k >= carry_k0 && k < carry_k0 + carry_n_k);
        if (!here) return fail(CAE_ERR_ARG, "cae_scene_blend: output rows %lld .. %lld need tile row %lld, which the call does not bring",
                               (long long)row0, (long long)row1, (long long)k);
    }
    SbArgs a;
    memset(&a, 0, sizeof a);
    a.pred_a = carry_pred, a.invalid_a = (const int*)carry_invalid, a.ka0 = (int)carry_k0, a.n_ka = (int)carry_n_k;
    a.pred_b = pred, a.invalid_b = (const int*)invalid, a.kb0 = (int)k0, a.n_kb = (int)n_k;
    a.n_y = (int)n_y, a.n_x = (int)n_x, a.n_t = (int)n_t_call, a.c_out = c_out, a.H = (int)H, a.W = (int)W;
    a.SY = (int)SY, a.SX = (geom->w - geom->ox) * geom->sx, a.LY = (int)LY, a.LX = (int)((geom->X - geom->w) * geom->sx);
    a.RY2 = 2 * geom->oy * geom->sy, a.RX2 = 2 * geom->ox * geom->sx;
    a.Xs = (int)Xs, a.row0 = (int)row0, a.row1 = (int)row1, a.out_c_stride = Ys * Xs, a.out_t_stride = out_t_stride;
    a.vmin = vmin, a.range = range, a.out = out, a.nan_pixels = (unsigned long long*)nan_pixels;
    // a workgroup per 256 columns and band of rows: about 8192 workgroups in all where the call is large enough
    const int64_t gx = (Xs + 255) / 256, gz = n_t_call * c_out, rows = row1 - row0;
    int64_t gy = 8192 / (gx * gz);
    gy = gy < 1 ? 1 : (gy > rows ? rows : gy);
    a.band = (int)((rows + gy - 1) / gy);
    gy = (rows + a.band - 1) / a.band;
    hipLaunchKernelGGL((k_scene_blend<SB_ROWS>), dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), dim3(256), 0, (hipStream_t)hip_stream, a);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
