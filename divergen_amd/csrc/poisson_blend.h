// Internal interface of poisson_blend.hip for the compositor (compositor.hip: dgx_copy_paste_blend_ws).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

constexpr int PB_REPORT_RECORDS = 32;      // one record per paste of a compositor call (K <= 31)
constexpr int PB_REPORT_DOUBLES = 4;       // (iterations, residual 2-norm, converged, |U|)
constexpr size_t PB_REPORT_BYTES = (size_t)PB_REPORT_RECORDS * PB_REPORT_DOUBLES * sizeof(double);

struct PbDesc { int32_t off, h, w, x0, y0; };

// Largest number of unknowns the workspace can hold (-1: it cannot even hold the image frame, or is misaligned / NULL).
int64_t pb_capacity(int H, int W, const void* work, size_t work_bytes);
// One paste, enqueued on `st`: descriptor from device memory (ddesc, 5 ints) when it is not NULL, else `hd`.  `record` is the index of
// the report record.  max_iter < 0: the bound of dgx_poisson_max_iter for `nmax`.  The caller has checked every argument.
int pb_enqueue(uint8_t* image, int H, int W, const uint8_t* src_rgba, const int32_t* ddesc, PbDesc hd, void* work, int64_t nmax,
               int max_iter, int record, hipStream_t st);
// Zero the report records of a call (pastes that are not 'possion' keep zeros).
int pb_clear_report(void* work, hipStream_t st);
