// group_kernels_gnn.hip -- the grouped row-block instances (group_kernels.h) for the PREBUILT GeneralNeuralNet shapes
// (element-wise output: last_act + loss, GNN:215-218, GNN:267-271), f32 and bf16: a translation unit of its own, as
// launch_small_gnn.hip is for the single-net instances, so that the two families compile side by side.
#include "static_shapes.h"

namespace gnn {
namespace host {

template <class SH, bool BF> static const void *rb_group_gnn(int act) {
    switch (act) {
    case 0: return reinterpret_cast<const void *>(&rowblock_group_kernel<SH, 0, 1, BF>);
    case 1: return reinterpret_cast<const void *>(&rowblock_group_kernel<SH, 1, 1, BF>);
    case 2: return reinterpret_cast<const void *>(&rowblock_group_kernel<SH, 2, 1, BF>);
    case 3: return reinterpret_cast<const void *>(&rowblock_group_kernel<SH, 3, 1, BF>);
    default: return reinterpret_cast<const void *>(&rowblock_group_kernel<SH, 4, 1, BF>);
    }
}

const void *rb_group_static_general(int which, int act, bool bf) {
    if (which == 0) return bf ? rb_group_gnn<RbMnistA, true>(act) : rb_group_gnn<RbMnistA, false>(act);
    return bf ? rb_group_gnn<RbMnistB, true>(act) : rb_group_gnn<RbMnistB, false>(act);
}

} // namespace host
} // namespace gnn
