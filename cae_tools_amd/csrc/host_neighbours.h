// host_neighbours.h - host only: novelty, the K nearest neighbours between two sets of rows: cae_case_neighbours over
// kernels_neighbours.h.  Included by stateless_host.h alone.
#pragma once

// Runs of reference tiles, one per workgroup of a query tile: about NB_RESIDENT workgroups in all where the call is large
// enough - two rounds of what the device holds at once, two workgroups on each of its 256 CUs by k_nb_tile's registers.  The
// order of the candidates is total, so the cut changes no result.
constexpr int64_t NB_RESIDENT = 1024;

static int64_t neighbours_tiles_per_split(int64_t n_query, int64_t n_ref) {
    const int64_t q_tiles = (n_query + NB_T - 1) / NB_T, r_tiles = (n_ref + NB_T - 1) / NB_T;
    int64_t want = (NB_RESIDENT + q_tiles - 1) / q_tiles;
    if (want > r_tiles) want = r_tiles;
    if (want > 65535) want = 65535;
    if (want < 1) want = 1;
    return (r_tiles + want - 1) / want;
}

static int64_t neighbours_splits(int64_t n_query, int64_t n_ref) {
    if (n_ref < 1) return 0;
    const int64_t per = neighbours_tiles_per_split(n_query, n_ref);
    return ((n_ref + NB_T - 1) / NB_T + per - 1) / per;
}

static bool neighbours_sizes_ok(int64_t n_query, int64_t n_ref, int k) {
    return n_query >= 0 && n_query <= 0x7fffffffLL && n_ref >= 0 && n_ref <= 0x7fffffffLL && k >= 1 && k <= NB_MAX_K;
}

// the workspace: the splits' partial lists, distances then indices, then the validity of the queries and of the references
static int64_t neighbours_part_entries(int64_t n_query, int64_t n_ref, int k) { return neighbours_splits(n_query, n_ref) * n_query * k; }

int64_t cae_case_neighbours_workspace_bytes(int64_t n_query, int64_t n_ref, int k) {
    if (n_query < 1 || !neighbours_sizes_ok(n_query, n_ref, k)) return 0;
    const int64_t e = neighbours_part_entries(n_query, n_ref, k);
    return e * 8 + (e + 1) / 2 * 8 + (n_query + n_ref + 1) / 2 * 8;
}

int cae_case_neighbours(const float* query, int64_t n_query, int64_t query_stride, const float* ref, int64_t n_ref, int64_t ref_stride,
                        int64_t dim, int k, int64_t ref_base, int64_t self_offset, int merge, double* dist2, int32_t* index,
                        int32_t* count, void* workspace, int64_t workspace_bytes, void* hip_stream) {
    if (!neighbours_sizes_ok(n_query, n_ref, k) || ref_base < 0 || ref_base + n_ref > 0x7fffffffLL || self_offset < -1 ||
        (merge != 0 && merge != 1))
        return fail(CAE_ERR_ARG, "cae_case_neighbours: bad argument (0 <= n_query, n_ref < 2^31, 1 <= k <= %d, 0 <= ref_base, ref_base + "
                                 "n_ref < 2^31, self_offset >= -1, merge 0 or 1)", NB_MAX_K);
    if ((n_query > 0 || n_ref > 0) && dim < 1) return fail(CAE_ERR_ARG, "cae_case_neighbours: dim must be at least 1 while rows exist");
    const CaseOperand Q{query, CAE_ELEM_F32, query_stride}, R{ref, CAE_ELEM_F32, ref_stride};
    if ((n_query > 0 && shorter(Q, dim)) || (n_ref > 0 && shorter(R, dim)))
        return fail(CAE_ERR_ARG, "cae_case_neighbours: a row stride is shorter than dim");
    if (!dist2 || !index || !count) return fail(CAE_ERR_ARG, "cae_case_neighbours: null output");
    if ((n_query > 0 && !Q.p) || (n_query > 0 && n_ref > 0 && !R.p)) return fail(CAE_ERR_ARG, "cae_case_neighbours: null operand with rows to read");
    if ((n_query > 0 && reaches(Q, n_query, dim)) || (n_ref > 0 && reaches(R, n_ref, dim)))
        return fail(CAE_ERR_ARG, "cae_case_neighbours: an operand reaches 2^60 elements from its pointer");
    if (any_misaligned({Q, R}) || ((uintptr_t)dist2 & 7) || ((uintptr_t)index & 3) || ((uintptr_t)count & 3))
        return fail(CAE_ERR_ARG, "cae_case_neighbours: pointers must be aligned to their element size");
    if (n_query == 0) return CAE_OK;
    const int64_t need = cae_case_neighbours_workspace_bytes(n_query, n_ref, k);
    if (workspace_short(workspace, workspace_bytes, need)) return no_workspace("cae_case_neighbours", need);
    if (n_ref == 0 && merge == 1) return CAE_OK;        // nothing joins the lists
    hipStream_t s = (hipStream_t)hip_stream;
    const int64_t entries = neighbours_part_entries(n_query, n_ref, k);
    NbArgs a;
    memset(&a, 0, sizeof a);
    a.q = query, a.r = ref, a.n_q = n_query, a.q_stride = query_stride, a.n_r = n_ref, a.r_stride = ref_stride, a.dim = dim;
    a.ref_base = ref_base, a.self_offset = self_offset, a.k = k, a.merge = merge;
    a.n_split = (int)neighbours_splits(n_query, n_ref);
    a.tiles_per_split = n_ref > 0 ? (int)neighbours_tiles_per_split(n_query, n_ref) : 0;
    a.part_d = (unsigned long long*)workspace;
    a.part_i = (int*)(a.part_d + entries);
    int* ok = a.part_i + (entries + 1) / 2 * 2;
    a.q_ok = ok, a.r_ok = ok + n_query;
    a.dist2 = dist2, a.index = (int*)index, a.count = (int*)count;
    hipLaunchKernelGGL((k_nb_valid<256>), dim3((unsigned)ceil_capped(n_query, 4, 8192)), dim3(256), 0, s, query, (long long)n_query,
                       (long long)query_stride, (long long)dim, ok);
    HIP_TRY(hipGetLastError());
    if (n_ref > 0) {
        hipLaunchKernelGGL((k_nb_valid<256>), dim3((unsigned)ceil_capped(n_ref, 4, 8192)), dim3(256), 0, s, ref, (long long)n_ref,
                           (long long)ref_stride, (long long)dim, ok + n_query);
        HIP_TRY(hipGetLastError());
        const dim3 grid((unsigned)((n_query + NB_T - 1) / NB_T), (unsigned)a.n_split);
        const size_t lds = (size_t)NB_TILE_BYTES + (size_t)k * NB_T * (sizeof(unsigned long long) + sizeof(int));      // at most 57 856 bytes
        hipLaunchKernelGGL((k_nb_tile<256>), grid, dim3(256), lds, s, a);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL((k_nb_merge<NB_T>), dim3((unsigned)((n_query + NB_T - 1) / NB_T)), dim3(NB_T), 0, s, a);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
