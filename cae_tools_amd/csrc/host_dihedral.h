// host_dihedral.h - host only: the eight symmetries of the square applied to packed rows, for augmentation between epochs and
// the self-ensemble of apply(): cae_dihedral_rows over kernels_dihedral.h.  Included by stateless_host.h alone.
#pragma once

// so many workgroups at the most; a workgroup takes one tile at a time and strides over the rest
constexpr int64_t DH_MAX_GROUPS = 16384;

int cae_dihedral_rows(const float* src, int64_t n_src, int c, int h, int w, float* dst, int64_t n_dst, const int32_t* row_dev,
                      const int32_t* code_dev, int group, void* hip_stream) {
    if (n_src < 0 || n_dst < 0 || c < 1 || h < 0 || w < 0 || (group != 4 && group != 8))
        return fail(CAE_ERR_ARG, "cae_dihedral_rows: bad argument (n_src >= 0, n_dst >= 0, c >= 1, h >= 0, w >= 0, group 4 or 8)");
    if (group == 8 && h != w) return fail(CAE_ERR_ARG, "cae_dihedral_rows: group 8 transposes, which needs square planes (h == w)");
    if (n_src > 0x7fffffffLL || n_dst > 0x7fffffffLL) return fail(CAE_ERR_ARG, "cae_dihedral_rows: more than 2^31 - 1 rows");
    if (n_dst == 0 || h == 0 || w == 0) return CAE_OK;
    if ((!src && n_src > 0) || !dst || !code_dev) return fail(CAE_ERR_ARG, "cae_dihedral_rows: null pointer");
    const __int128 per = (__int128)c * h * w;
    if (n_src * per > ((__int128)1 << 60) || n_dst * per > ((__int128)1 << 60))
        return fail(CAE_ERR_ARG, "cae_dihedral_rows: an operand reaches 2^60 elements from its pointer");
    if (((uintptr_t)src & 3) || ((uintptr_t)dst & 3) || ((uintptr_t)row_dev & 3) || ((uintptr_t)code_dev & 3))
        return fail(CAE_ERR_ARG, "cae_dihedral_rows: pointers must be 4-byte aligned");
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)(n_src * per) * 4, d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)(n_dst * per) * 4;
    if (s0 < d1 && d0 < s1) return fail(CAE_ERR_ARG, "cae_dihedral_rows: dst overlaps src");
    DhArgs a;
    memset(&a, 0, sizeof a);
    a.src = (const unsigned*)src, a.dst = (unsigned*)dst, a.row = (const int*)row_dev, a.code = (const int*)code_dev;
    a.n_src = n_src, a.c = c, a.h = h, a.w = w, a.group = group;
    a.tiles_x = ((int64_t)w + DH_TILE - 1) / DH_TILE;
    a.tiles_plane = a.tiles_x * (((int64_t)h + DH_TILE - 1) / DH_TILE);
    a.items = n_dst * c * a.tiles_plane;
    const dim3 grid((unsigned)(a.items < DH_MAX_GROUPS ? a.items : DH_MAX_GROUPS));
    hipLaunchKernelGGL((k_dihedral_rows<DH_WAVES>), grid, dim3(64 * DH_WAVES), 0, (hipStream_t)hip_stream, a);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
