// rowerr.hpp -- the per-row arithmetic of the reference's compute_epe_test (utils_eval.py:162-180), shared by the two
// kernels that evaluate flows: seq_metrics_kernel (seqeval.hip: sums per gap and class) and seg_chunk_kernel (segeval.hip:
// sums per segment).  fp64 with numpy's operation order; the files that include this are compiled with -ffp-contract=off
// (build.py: CFLAGS), so the squares, the two additions, the square root and the division are the separately rounded
// operations numpy performs, the square root correctly rounded and the division IEEE.
// crop_keep is the row test of the kernels that walk a whole sample: seq_metrics_kernel, class_table_kernel (classeval.hip:
// counts and sums per class, speed bucket and error split) and bucket_table_kernel (bucketeval.hip: per class and speed bucket,
// with a table per workgroup).  The last two also share the rules below it: a row's speed, its class row, its bucket, and the
// grid that follows from the number of rows.
#pragma once
#include <hip/hip_runtime.h>

namespace icpflow {

struct Crop {
    int mode;                // ICPFLOW_SEQ_CROP_*
    double rx, ry, zmin;
};

// crop_data, utils_eval.py:33-38 (a NaN coordinate fails every comparison there and here); mode 0 / 1 / 2 are
// ICPFLOW_SEQ_CROP_NONE / _XY / _XYZ
__device__ __forceinline__ bool crop_keep(const Crop &crop, double x, double y, double z)
{
    return crop.mode == 0 || (fabs(x) < crop.rx && fabs(y) < crop.ry && (crop.mode == 1 || z > crop.zmin));
}

struct RowError {
    double e, r;             // end point error, relative error
    bool p0, p1, p2, p3;     // strict, relax, outlier, Routlier
};

// utils_eval.py:170-180 on a row's e and r
__device__ __forceinline__ RowError row_predicates(double e, double r)
{
    return RowError{e, r, e < 0.05 || r < 0.05, e < 0.1 || r < 0.1, e > 0.3 || r > 0.1, e > 0.3 && r > 0.3};
}

// utils_eval.py:163-168: numpy's norm is sqrt((x*x + y*y) + z*z), each operation rounded; the predicted flow is float32,
// widened (exact)
__device__ __forceinline__ RowError row_error(double gx, double gy, double gz, float px, float py, float pz)
{
    const double dx = gx - (double)px, dy = gy - (double)py, dz = gz - (double)pz;
    const double e = sqrt((dx * dx + dy * dy) + dz * dz);
    const double r = e / (sqrt((gx * gx + gy * gy) + gz * gz) + 1e-20);
    return row_predicates(e, r);
}

// |gt| in metres per frame: numpy's norm, every operation rounded by itself
__device__ __forceinline__ double row_speed(double gx, double gy, double gz)
{
    return sqrt((gx * gx + gy * gy) + gz * gz);
}

// the class row of a value: an integer value of [class_lo, class_lo + G - 2], else the last row (NaN fails every comparison)
__device__ __forceinline__ int class_row(double v, double class_lo, int G)
{
    int g = G - 1;
    if (v == floor(v) && v >= class_lo && v <= class_lo + (double)(G - 2)) g = (int)(v - class_lo);
    return g;
}

// the bucket of a value among n ascending interior edges: the number of edges <= v (lower edge inclusive; a NaN is bucket 0)
__device__ __forceinline__ int edge_bucket(double v, const double *edge, int n)
{
    int s = 0;
    for (int k = 0; k < n; ++k) s += v >= edge[k] ? 1 : 0;
    return s;
}

// the grid of the two table kernels: a workgroup of kTableThreads threads per kTableThreads * kTableRowsPerThread rows, at
// least one and at most kTableMaxGrid (a CU each) -- a function of m alone, never of the device
constexpr int kTableThreads = 256;
constexpr int kTableRowsPerThread = 8;
constexpr int kTableMaxGrid = 256;
inline int table_grid(int m)
{
    const long long per = (long long)kTableThreads * kTableRowsPerThread;
    const long long g = ((long long)m + per - 1) / per;
    return (int)(g < 1 ? 1 : g > kTableMaxGrid ? kTableMaxGrid : g);
}

}  // namespace icpflow
