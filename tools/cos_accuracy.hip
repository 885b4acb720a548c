// Probe: accuracy of v_cos_f32 (input in revolutions) on gfx950, against fp64 -- the cosine of the jet trunk's activation derivative
// (siren_trunk_f32_jet.hip.h), as tools/sin_accuracy.hip measured the sine: with an explicit range reduction and directly, over
// [-0.5, 0.5] and [-32, 32] revolutions, and what sin_rev(r + 1/4) would give instead (the phase rounded in fp32).
// Build+run on the GPU box:  hipcc --offload-arch=gfx950 -O2 tools/cos_accuracy.hip -o /tmp/cosacc && /tmp/cosacc
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

__global__ void k(const float* x, float* reduced, float* direct, float* shifted_sine, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        float r = x[i];
        float f = r - __builtin_rintf(r);
        reduced[i] = __builtin_amdgcn_cosf(f);
        direct[i] = __builtin_amdgcn_cosf(r);
        shifted_sine[i] = __builtin_amdgcn_sinf(r + 0.25f);
    }
}

#define CHECK(e) do { hipError_t err_ = (e); if (err_ != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(err_)); return 1; } } while (0)

int main() {
    const int n = 1 << 22;
    std::vector<float> x(n), c(n), d(n), s(n);
    for (int i = 0; i < n; ++i) {
        double t = (double)i / n;
        x[i] = (float)((i & 1) ? (t - 0.5) : (t - 0.5) * 64.0);  // [-0.5,0.5] and [-32,32] revolutions
    }
    float *dx, *dc, *dd, *ds;
    CHECK(hipMalloc(&dx, n * 4)); CHECK(hipMalloc(&dc, n * 4)); CHECK(hipMalloc(&dd, n * 4)); CHECK(hipMalloc(&ds, n * 4));
    CHECK(hipMemcpy(dx, x.data(), n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k, dim3(n / 256), dim3(256), 0, 0, dx, dc, dd, ds, n);
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(c.data(), dc, n * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(d.data(), dd, n * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(s.data(), ds, n * 4, hipMemcpyDeviceToHost));
    double m_small = 0, m_big = 0, m_big_direct = 0, m_big_shift = 0, m_small_shift = 0;
    for (int i = 0; i < n; ++i) {
        double ref = std::cos(2.0 * M_PI * (double)x[i]);
        double e_red = std::fabs((double)c[i] - ref), e_dir = std::fabs((double)d[i] - ref), e_sh = std::fabs((double)s[i] - ref);
        if (i & 1) { m_small = std::fmax(m_small, e_dir); m_small_shift = std::fmax(m_small_shift, e_sh); }
        else { m_big = std::fmax(m_big, e_red); m_big_direct = std::fmax(m_big_direct, e_dir); m_big_shift = std::fmax(m_big_shift, e_sh); }
    }
    printf("v_cos_f32 max abs err: |r|<=0.5 direct %.3e ; |r|<=32 reduced %.3e ; |r|<=32 direct %.3e\n", m_small, m_big, m_big_direct);
    printf("v_sin_f32(r + 0.25f) as a cosine: |r|<=0.5 %.3e ; |r|<=32 %.3e\n", m_small_shift, m_big_shift);
    return 0;
}
