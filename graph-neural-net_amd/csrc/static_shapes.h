// static_shapes.h -- the shapes with PREBUILT compile-time plans (BASELINE.json's two MNIST nets) and the tables of their
// kernel instances.  launch_small.hip instantiates the SoftmaxCrossEntropyNeuralNet forms (OUTK = 0), launch_small_gnn.hip
// the GeneralNeuralNet forms (OUTK = 1: last_act + loss, GNN:215-218, GNN:267-271) -- two translation units so that the two
// families compile side by side (each is ~70 s of hipcc); the grouped row-block instances likewise in group_kernels.hip and
// group_kernels_gnn.hip, their sized twins in group_kernels_sized.hip and group_kernels_sized_gnn.hip.  The tables are function templates over the choices of instances.h: a unit compiles what it asks for.
#pragma once
#include "instances.h"

namespace gnn {
namespace host {

using ShapeMnistA = StaticShape<784, 300, 100, 10>;
using ShapeMnistB = StaticShape<784, 100, 50, 10>;
using RbMnistA = RbStaticShape<784, 300, 100, 10>;
using RbMnistB = RbStaticShape<784, 100, 50, 10>;

// which: 0 = 784-300-100-10, 1 = 784-100-50-10; the choices themselves: instances.h
// middle4_kernel table: [shape][activation][output kind][variant]
template <int OUTK> const void *mid4_static_table(int which, int act, int variant) {
    return with_act(act, [&](auto A) {
        constexpr int a = decltype(A)::value;
        return which == 0 ? mid4_variant<ShapeMnistA, a, OUTK>(variant) : mid4_variant<ShapeMnistB, a, OUTK>(variant);
    });
}
// row-block table: [family: single net / group][shape][activation][output kind][dtype]
template <class Fam, int OUTK> const void *rb_static_table(int which, int act, bool bf) {
    return with_act(act, [&](auto A) {
        constexpr int a = decltype(A)::value;
        if (which == 0) return bf ? Fam::template fn<RbMnistA, a, OUTK, true>() : Fam::template fn<RbMnistA, a, OUTK, false>();
        return bf ? Fam::template fn<RbMnistB, a, OUTK, true>() : Fam::template fn<RbMnistB, a, OUTK, false>();
    });
}

// the OUTK = 1 tables: launch_small_gnn.hip, group_kernels_gnn.hip
const void *mid4_static_general(int which, int act, int variant);
const void *rb_static_general(int which, int act, bool bf);
const void *rb_group_static_general(int which, int act, bool bf);
const void *rb_group_sized_static_general(int which, int act, bool bf); // (group_kernels_sized_gnn.hip)

} // namespace host
} // namespace gnn
