// group_kernels_sized_gnn.hip -- the SIZED grouped row-block instances (group_kernels.h) for the PREBUILT GeneralNeuralNet shapes,
// f32 and bf16: a translation unit of its own, as group_kernels_gnn.hip is for the uniform ones.
#include "static_shapes.h"

namespace gnn {
namespace host {

const void *rb_group_sized_static_general(int which, int act, bool bf) { return rb_static_table<RbGroupSized, 1>(which, act, bf); }

} // namespace host
} // namespace gnn
