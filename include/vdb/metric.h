// vdb/metric.h — distance metric ordinals of the reference (engine/kernels.cuh:24-28),
// without any device headers. L2 = squared L2, InnerProduct = negated dot product,
// Cosine = the reference CPU path's behaviour (distance 0.0f, ivf_flat_index.cpp:351-362).
//
// CosineDistance (3, appended: 0, 1 and 2 keep their ordinals) is this engine's own: true
// cosine distance 1 - cos(query, row), served as an inner-product index over unit rows. Rows
// are normalised once when they enter the index, queries when they enter a batch, and a
// distance is reported as 1.0f + (-dot); entries stay ordered by (-dot, id). The norm is a
// fixed-order fp32 sum, a correctly rounded sqrt and a correctly rounded division, and a row
// whose norm is zero, infinite or NaN is kept as it is (include/vdb_ivf.h has the exact rule).
// This deliberately differs from the reference's unported GPU functor (kernels.cuh:63-80): no
// + 1e-8 epsilon, no per-pair norms.
#pragma once

namespace vdb {
namespace kernels {
enum class Metric { L2, InnerProduct, Cosine, CosineDistance };
}  // namespace kernels
}  // namespace vdb
