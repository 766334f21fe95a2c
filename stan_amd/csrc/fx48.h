// fx48.h -- the FIXED-48 value stream's number format, shared by who writes it (matrix_streams.hip: k_to_fx48) and who
// reads it (spmv_kernels.inc: load9 and the products' x * 2^-46): a value a, |a| < 2, travels as round(a * 2^46) + 2^47.
#pragma once

constexpr double FX48_ONE = 70368744177664.0;                          // 2^46
constexpr double FX48_INV = 1.0 / 70368744177664.0;                    // 2^-46
constexpr double FX48_BIAS = 4503599627370496.0 + 140737488355328.0;   // 2^52 + 2^47
