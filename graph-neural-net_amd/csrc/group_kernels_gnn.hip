// group_kernels_gnn.hip -- the grouped row-block instances (group_kernels.h) for the PREBUILT GeneralNeuralNet shapes
// (element-wise output: last_act + loss, GNN:215-218, GNN:267-271), f32 and bf16: a translation unit of its own, as
// launch_small_gnn.hip is for the single-net instances, so that the two families compile side by side: the row-block table of
// static_shapes.h asked for the grouped family and OUTK = 1.
#include "static_shapes.h"

namespace gnn {
namespace host {

const void *rb_group_static_general(int which, int act, bool bf) { return rb_static_table<RbGroup, 1>(which, act, bf); }

} // namespace host
} // namespace gnn
