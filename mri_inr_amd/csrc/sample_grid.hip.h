// Layer 0 of the 16-bit trunks for a coordinate set that is not the model's own grid.
//
// The split-fp16 trunks (H = 256: f16x3n / f16x3h / f16x3w) and the single-product ones (H = 512: x1n / x1w) do not evaluate layer 0;
// they read   S0T[f/4][q][f%4] = act0(w0_initial * (W0 x_q + b0))   from a table (siren_trunk_f16_common.hip.h).  For the model's own
// grid msiren_commit_weights builds it on the host (weights_pack.hip).  A call that brings its own coordinates (msiren_sample_*, the
// *_scaled slice pipeline) needs its own table in front of its trunk, on its stream: a host build of 256 x 2 304 fp64 sines takes
// ~20 ms, twenty times the trunk work it would feed.  Hence this kernel.
//
// Arithmetic: that of the host loop, operation for operation.  The pre-activation is formed in fp32 with two fmaf in F.linear's
// order (bias, then column 0, then column 1); the activation in fp64 -- sin(w0_initial * pre), Morlet: * exp(-0.5 * pre * pre) -- and
// rounded ONCE to fp32.  FMA contraction is OFF for the kernel's own expressions (the pragma below), so every fp64 product and the
// final Morlet product are rounded on their own as on the host; the two fmaf are explicit.  The device library's fp64 sin / exp are
// not the host libm's: an entry may differ from the committed table's in its last fp32 bit where the fp64 value lies within the two
// libraries' error of a rounding boundary (measured: LAB_NOTES.md section 13).
//
// One thread per (feature group of 4, coordinate): consecutive threads store consecutive float4 along Q, W0 / b0 are wave-uniform
// unless a wave straddles two groups.  No atomics; every element is written by exactly one thread.
#pragma once
#include <hip/hip_runtime.h>

namespace msiren {

struct Layer0TableParams {
    const float* coords;  // (Q, 2): row coordinate, column coordinate
    const float* w0;      // net.layers.0.weight (H, 2) as stored
    const float* b0;      // net.layers.0.bias (H) as stored; zeros for a model without bias
    float* table;         // (H/4, Q, 4)
    int Q, groups;        // groups = H/4
    float w0_initial;
    int morlet;
};

__global__ __launch_bounds__(256) void layer0_table_kernel(Layer0TableParams p) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)p.groups * p.Q) return;
    const int g = (int)(i / p.Q), q = (int)(i - (int64_t)g * p.Q);
    const float2 xy = reinterpret_cast<const float2*>(p.coords)[q];
    const float4 wa = reinterpret_cast<const float4*>(p.w0)[2 * g], wb = reinterpret_cast<const float4*>(p.w0)[2 * g + 1];
    const float4 b = reinterpret_cast<const float4*>(p.b0)[g];
    const float wx[4] = {wa.x, wa.z, wb.x, wb.z}, wy[4] = {wa.y, wa.w, wb.y, wb.w}, bb[4] = {b.x, b.y, b.z, b.w};
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float pre = __builtin_fmaf(xy.y, wy[j], __builtin_fmaf(xy.x, wx[j], bb[j]));
        double a = sin((double)p.w0_initial * (double)pre);
        if (p.morlet) a *= exp(-0.5 * (double)pre * (double)pre);
        o[j] = (float)a;
    }
    reinterpret_cast<float4*>(p.table)[i] = make_float4(o[0], o[1], o[2], o[3]);
}

}  // namespace msiren
