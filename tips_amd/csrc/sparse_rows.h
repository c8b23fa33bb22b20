// sparse_rows.h — launchers of the ordered row-sum kernels (sparse_rows.hip).
// Internal to libtips_hip.so (not part of the C-ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tips {

// Bytes of the workspace launch_rows_sum needs for `rows` dense rows and `n` entries:
// offset[rows + 1] and cursor[rows + 1] (8 B each), then the placed and the ordered entry ids
// (8 B each per entry): 8 (2 rows + 2) + 16 n.
inline int64_t rows_sum_workspace_bytes(int64_t rows, int64_t n) { return 8 * (2 * rows + 2) + 16 * n; }

// dst[rows][row_elems] = post * (ordered sum over the entries e with indices[e] == row of pre *
// values[e][:]), entries in ascending e, folded left to right from the first one in the working type
// (fp32 for f32 / f16 / bf16, f64 for f64, the integer type itself), rounded once at the store; a row
// nothing names is +0. An entry whose index is outside [0, rows) is skipped and counted
// (rows_sum_bad_indices). pre == post == 1: no multiply at all; other factors: float dtypes only.
// Every row of dst is written exactly once. workspace: device memory of rows_sum_workspace_bytes,
// 8-B aligned. Stream-ordered on s; rows, row_elems > 0, n >= 0.
hipError_t launch_rows_sum(void* dst, int64_t rows, int64_t row_elems, const void* values, const int64_t* indices,
                           int64_t n, int dtype, double pre, double post, void* workspace, hipStream_t s);

// The current device's count of skipped entries since the library was loaded. Synchronises the device.
hipError_t rows_sum_bad_indices(int64_t* out);

}  // namespace tips
