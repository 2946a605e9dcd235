// stateless_host.h - host only: the entry points of cae_hip.h that use no engine.  Their shared vocabulary, then one host_*.h per
// subject in the order the subjects were added: a kernel template sits in the code object where its entry point instantiates it.
#pragma once
#include <initializer_list>
#include <type_traits>

// ---- the vocabulary of the entry points below: element kinds, case operands, grid sizes ---------------

static int elem_bytes(int kind) { return kind == CAE_ELEM_F32 || kind == CAE_ELEM_F32_BE ? 4 : 8; }
static bool kind_known(int kind) { return kind >= CAE_ELEM_F32 && kind <= CAE_ELEM_F64_BE; }

// One operand of a case kernel: channel 0 of the cases, `stride` elements from one case to the next.  The checks are
// functions over it; each entry point calls the ones it has always called, in its own order and under its own texts.
struct CaseOperand {
    const void* p;
    int kind;
    int64_t stride;
};
static bool known(const CaseOperand& o) { return kind_known(o.kind); }
static bool shorter(const CaseOperand& o, int64_t plane) { return o.stride < plane; }
static bool misaligned(const CaseOperand& o) { return (uintptr_t)o.p % elem_bytes(o.kind) != 0; }
// the last case ends above 2^60 elements from the pointer; in 128 bits, so that no stride, however large, wraps the product
static bool reaches(const CaseOperand& o, int64_t n_case, int64_t plane) {
    return (__int128)(n_case - 1) * o.stride + plane > ((__int128)1 << 60);
}
// an operand the caller may leave out (NULL): its kind and stride are then not looked at
static CaseOperand optional_operand(const void* p, int kind, int64_t stride) {
    return {p, p ? kind : CAE_ELEM_F32, p ? stride : 0};
}

// The three rungs most entry points share, each over a short list of operands, those with a plane of their own beside it.
// An optional operand that was not given (p NULL) is skipped here, not by the caller; the others the caller has refused as
// null before.  The fail(...) lines, their order and whatever else a rung tests stay with the entry point.
struct OnPlane { CaseOperand o; int64_t plane; };
static bool any_shorter(std::initializer_list<OnPlane> l) {
    return std::any_of(l.begin(), l.end(), [](const OnPlane& e) { return e.o.p && shorter(e.o, e.plane); });
}
static bool any_reaches(int64_t n_case, std::initializer_list<OnPlane> l) {
    return std::any_of(l.begin(), l.end(), [&](const OnPlane& e) { return e.o.p && reaches(e.o, n_case, e.plane); });
}
static bool any_misaligned(std::initializer_list<CaseOperand> l) { return std::any_of(l.begin(), l.end(), misaligned); }

// no workspace of `need` bytes, 8 bytes aligned
static bool workspace_short(const void* ws, int64_t bytes, int64_t need) { return !ws || bytes < need || ((uintptr_t)ws & 7); }

// the refusal for it, which names the entry point's size function
static int no_workspace(const char* who, int64_t need) {
    return fail(CAE_ERR_ARG, "%s: needs a workspace of %lld bytes (%s_workspace_bytes)", who, (long long)need, who);
}

// neither NaN nor infinite
static bool is_finite(double x) { return x - x == 0.0; }

// ceil(n / per), at most cap: so many workgroups for n items (the grid-stride kernels walk the rest)
static int64_t ceil_capped(int64_t n, int64_t per, int64_t cap) {
    const int64_t b = (n + per - 1) / per;
    return b < cap ? b : cap;
}

// The kind dispatch: f(std::integral_constant<int, K>()) for the run-time element kind, which the caller has checked
// (kind_known).  The kind-templated kernels are instantiated through it alone, the kinds in ascending order and "none"
// last, as the switches it replaces had them: a kernel's place in the code object follows the order of instantiation,
// and moving code inside the code object has cost the training step time before.
template <class F>
static void with_kind(int kind, F&& f) {
    switch (kind) {
    case CAE_ELEM_F32: f(std::integral_constant<int, 0>()); break;
    case CAE_ELEM_F32_BE: f(std::integral_constant<int, 1>()); break;
    case CAE_ELEM_F64: f(std::integral_constant<int, 2>()); break;
    default: f(std::integral_constant<int, 3>()); break;
    }
}

// two operands: f(KP, KA), the first the outer switch
template <class F>
static void with_kinds(int kind_p, int kind_a, F&& f) {
    with_kind(kind_p, [&](auto KP) { with_kind(kind_a, [&](auto KA) { f(KP, KA); }); });
}

// the same for an optional operand: kind -1 stands for "none"
template <class F>
static void with_kind_or_none(int kind, F&& f) {
    switch (kind) {
    case CAE_ELEM_F32: f(std::integral_constant<int, 0>()); break;
    case CAE_ELEM_F32_BE: f(std::integral_constant<int, 1>()); break;
    case CAE_ELEM_F64: f(std::integral_constant<int, 2>()); break;
    case CAE_ELEM_F64_BE: f(std::integral_constant<int, 3>()); break;
    default: f(std::integral_constant<int, -1>()); break;
    }
}

// The width dispatch of the kernels templated over element bytes: f(WP, WA, WS), the widths of three operands as
// std::integral_constant<int, 4 or 8>, 0 for a third that is not there.  The first operand is the outer switch, 4 before 8.
template <class F>
static void with_widths(const CaseOperand& P, const CaseOperand& A, const CaseOperand& S, F&& f) {
    auto third = [&](auto WP, auto WA) {
        if (!S.p) f(WP, WA, std::integral_constant<int, 0>());
        else if (elem_bytes(S.kind) == 4) f(WP, WA, std::integral_constant<int, 4>());
        else f(WP, WA, std::integral_constant<int, 8>());
    };
    auto second = [&](auto WP) {
        if (elem_bytes(A.kind) == 4) third(WP, std::integral_constant<int, 4>());
        else third(WP, std::integral_constant<int, 8>());
    };
    if (elem_bytes(P.kind) == 4) second(std::integral_constant<int, 4>());
    else second(std::integral_constant<int, 8>());
}

// Launches Kernel(a) with `lds` bytes of dynamic LDS.  Above 64 KiB a kernel has to ask: `granted` belongs to the
// instantiation, so each kernel asks once per size it has not yet been given.
template <auto Kernel, class Args>
static void launch_with_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args& a) {
    static size_t granted = 64 * 1024;
    if (lds > granted) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        granted = lds;
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, s, a);
}

// ---- the entry points by subject (the order is the order of the kernels in the code object) -----------

#include "host_loader.h"
#include "host_case_measures.h"
#include "host_ensemble.h"
#include "host_case_pages.h"
#include "host_pixel_sums.h"
#include "host_spectra.h"
#include "host_ssim.h"
#include "host_baseline.h"
#include "host_scene.h"
// the last sections: their kernels are emitted after every other kernel of the code object
#include "host_hist.h"
#include "host_strata.h"
#include "host_fss.h"
#include "host_importance.h"
#include "host_quantile.h"
#include "host_neighbours.h"
#include "host_residual.h"
#include "host_compare.h"
#include "host_dihedral.h"
#include "host_blend.h"
