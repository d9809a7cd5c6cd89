// instances.h -- internal, host only: the ONE table of the small-net kernel instances.  A kernel instance is chosen from
// run-time values (shape, layer count, activation, output kind, dtype, step form, single net or group); every such choice
// is written here once, and the units that instantiate the kernels (launch_small*.hip, group_kernels*.hip; launch_gemm.hip
// includes it for with_act alone, in launch_fwd_first) call it with the template arguments THEY own -- a function template below
// instantiates nothing until a unit uses it, so which unit compiles which kernels is decided by the callers alone.
// A new kernel form is added here, once; launch_instance (handle.h) is the one launcher of what these functions return.
#pragma once
#include "handle.h"

#include <type_traits>

namespace gnn {
namespace host {

#define GNN_KERNEL(...) reinterpret_cast<const void *>(&__VA_ARGS__) // a kernel instance as hipLaunchKernel takes it

template <int V> using int_c = std::integral_constant<int, V>;

// f(int_c<A>{}) for the activation as a template argument: 0..3, anything else 4 (identity)
template <class F> auto with_act(int act, F f) {
    switch (act) {
    case 0: return f(int_c<0>{});
    case 1: return f(int_c<1>{});
    case 2: return f(int_c<2>{});
    case 3: return f(int_c<3>{});
    default: return f(int_c<4>{});
    }
}

// f(int_c<NL>{}) for the layer count as a template argument: 3..6, anything else 0 (the count stays a kernel argument)
template <class F> auto with_layer_count(int L, F f) {
    switch (L) {
    case 3: return f(int_c<3>{});
    case 4: return f(int_c<4>{});
    case 5: return f(int_c<5>{});
    case 6: return f(int_c<6>{});
    default: return f(int_c<0>{});
    }
}

// ---- middle4_kernel ------------------------------------------------------------------------------
// variant: 0 forward only, 1 forward + backward, 2 forward + backward with A_1 from the K slabs of tile_step_kernel, 3 = 2 in bf16
template <class SH, int ACT, int OUTK> const void *mid4_variant(int variant) {
    return variant == 3   ? GNN_KERNEL(middle4_kernel<SH, ACT, OUTK, true, true, true>)
           : variant == 2 ? GNN_KERNEL(middle4_kernel<SH, ACT, OUTK, true, true>)
           : variant == 1 ? GNN_KERNEL(middle4_kernel<SH, ACT, OUTK, true>)
                          : GNN_KERNEL(middle4_kernel<SH, ACT, OUTK, false>);
}

// runtime extents: layer count templated, activation read from the arguments
template <int OUTK> const void *mid4_runtime_instance(int L, int variant) {
    return with_layer_count(L, [&](auto NL) { return mid4_variant<RuntimeShape<decltype(NL)::value>, -1, OUTK>(variant); });
}

// ---- the row-block kernel: a family names the kernel template (single net / group / group with sizes) ----
struct RbSingle {
    template <class SH, int ACT, int OUTK, bool BF> static const void *fn() { return GNN_KERNEL(rowblock_kernel<SH, ACT, OUTK, BF>); }
};
struct RbGroup {
    template <class SH, int ACT, int OUTK, bool BF> static const void *fn() { return GNN_KERNEL(rowblock_group_kernel<SH, ACT, OUTK, BF>); }
};
struct RbGroupSized { // (one batch size per member: group_kernels.h)
    template <class SH, int ACT, int OUTK, bool BF> static const void *fn() { return GNN_KERNEL(rowblock_group_sized_kernel<SH, ACT, OUTK, BF>); }
};

// runtime extents; the bf16 form exists for nets of three and four layers.  Null otherwise, for both families: plan_rowblock
// returns before it asks for a deeper bf16 net, and make_rb_plan refuses L < 3 for every dtype (rowblock_kernel.h)
template <class Fam, int OUTK> const void *rb_runtime_instance(int L, bool bf) {
    if (bf) {
        return L == 3   ? Fam::template fn<RbRuntimeShape<3>, -1, OUTK, true>()
               : L == 4 ? Fam::template fn<RbRuntimeShape<4>, -1, OUTK, true>()
                        : nullptr;
    }
    return with_layer_count(L, [](auto NL) { return Fam::template fn<RbRuntimeShape<decltype(NL)::value>, -1, OUTK, false>(); });
}

// ---- the tile-owner kernel: (gsrc, gdst, fwd) as in tile_step_kernel.h -------------------------------------
// A family names the kernel template and says whether it has the peer forms (GSRC 3 / 4: dp.hip); a family without them
// gets null for those (the grouped kernels static_assert GSRC <= 2, so they are not even named).  The single-net families are
// templates on HEAD (launch_small.hip): the head-argument prologue of tile_step_kernel.h, or, GNN_MLP_TILE_HEAD=0, the earlier one.  gdst is read only with
// gsrc == 1, fwd not with gsrc == 0 or <1, 1>: the callers pass (0, 0, .), (1, 1, .), (1, 2, .), (2..4, 2, .) only.
template <class Fam> const void *tile_step_instance(int gsrc, int gdst, bool fwd) {
    auto fwd_or_not = [&](auto S) {
        constexpr int s = decltype(S)::value;
        return fwd ? Fam::template fn<s, 2, true>() : Fam::template fn<s, 2, false>();
    };
    if (gsrc == 0) return Fam::template fn<0, 0, true>();
    if (gsrc == 1 && gdst == 1) return Fam::template fn<1, 1, false>();
    if (gsrc == 1) return fwd_or_not(int_c<1>{});
    if (gsrc == 2) return fwd_or_not(int_c<2>{});
    if constexpr (Fam::kPeerForms) return gsrc == 3 ? fwd_or_not(int_c<3>{}) : fwd_or_not(int_c<4>{});
    else return nullptr;
}

// the ONE instance that knows the workgroup kinds of the merged map (tile_step_kernel.h, make_merged_tile_map): the training
// form <1, 2, true> of a single f32 net with the head prologue.  Every other form keeps the one-tile-per-workgroup map.
template <class Fam> const void *tile_step_merged_instance() { return Fam::merged(); }

} // namespace host
} // namespace gnn
