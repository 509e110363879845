// Device loss meter: fold the scalars of one training step (the 0-dim loss tensors, the optimizer's total_norm and gscale) into running
// statistics without a read-back. One launch of one wave; lane i owns source i and the table row row_of[i] (the host refuses two
// sources on one row, so no two lanes touch the same row). The source pointers and row indices travel as kernel arguments: no
// host -> device copy, no pointer table in device memory.
//   row = [last, ema, sum, count, min, max, nonfinite, reserved]; the host initialises it to [0, 0, 0, 0, +inf, -inf, 0, 0]
//   x = *src[i]:  last = x always; x not finite: nonfinite += 1 and nothing else; otherwise
//   ema = count == 0 ? x : x * take + ema * keep (two roundings of the products, one of the sum: no FMA contraction, so a numpy float32
//   restatement is bit-equal), sum += x, count += 1, min = fminf(min, x), max = fmaxf(max, x).
// RunningMeter of the reference (utils/logger.py:72-85) is ema with keep = 0.99, take = 1 - 0.99.
#include "common.h"
#include "../../include/valor_hip.h"

struct MeterArgs {
    const float* src[VALOR_METER_MAX_SRC];
    int32_t row[VALOR_METER_MAX_SRC];
};

__global__ __launch_bounds__(64) void meter_update_kernel(float* table, MeterArgs a, int n, float keep, float take) {
    const int i = threadIdx.x;
    if (i >= n) return;
    const float x = *a.src[i];
    f32x4_t* row = (f32x4_t*)(table + (int64_t)a.row[i] * VALOR_METER_FIELDS);
    f32x4_t lo = row[0], hi = row[1];           // lo = last, ema, sum, count ; hi = min, max, nonfinite, reserved
    lo[0] = x;
    const bool finite = (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
    if (finite) {
        lo[1] = lo[3] == 0.f ? x : __fadd_rn(__fmul_rn(x, take), __fmul_rn(lo[1], keep));
        lo[2] = __fadd_rn(lo[2], x);
        lo[3] = __fadd_rn(lo[3], 1.f);
        hi[0] = fminf(hi[0], x);
        hi[1] = fmaxf(hi[1], x);
    } else {
        hi[2] = __fadd_rn(hi[2], 1.f);
    }
    row[0] = lo;
    row[1] = hi;
}

extern "C" int valor_meter_update(void* stream, float* table, int rows, const float* const* src, const int32_t* row_of, int n,
                                  float keep, float take) {
    if (n < 0 || n > VALOR_METER_MAX_SRC) return VALOR_ERR_ARG;
    if (n == 0) return VALOR_OK;
    if (rows < 1 || !table || !src || !row_of || ((uintptr_t)table & 15)) return VALOR_ERR_ARG;
    MeterArgs a;
    for (int i = 0; i < n; i++) {
        if (!src[i] || ((uintptr_t)src[i] & 3) || row_of[i] < 0 || row_of[i] >= rows) return VALOR_ERR_ARG;
        for (int j = 0; j < i; j++)                 // two lanes on one row would race
            if (row_of[j] == row_of[i]) return VALOR_ERR_ARG;
        a.src[i] = src[i];
        a.row[i] = row_of[i];
    }
    for (int i = n; i < VALOR_METER_MAX_SRC; i++) {
        a.src[i] = nullptr;
        a.row[i] = 0;
    }
    hipLaunchKernelGGL(meter_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, table, a, n, keep, take);
    return valor_launch_status();
}
