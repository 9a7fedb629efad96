// kernels_icp.hip -- dense point-to-plane ICP with projective association (slr_cloud_normals, slr_icp_linearize,
// slr_register_icp): a source point set is registered against a target cloud organised on its camera grid.  A source point finds
// its target by projecting into the target's pinhole grid, so there is no search structure: one streaming pass per iteration.
// gfx950 (MI355X) only.  include/slr.h gives the exact rule; tests/np_icp_model.py restates it in NumPy.
//
// Passes (one launch each, on the ctx stream):
//   normals    one thread per target pixel: central differences of the four neighbours, all in f64 (bit-exact against the model:
//              every operation is a correctly rounded f64 add / mul / div / sqrt, and the library is built with -ffp-contract=off);
//   linearise  one thread per source point (a grid-stride loop over a grid that depends on n_src only): transform, project, gate,
//              and accumulate the 21 upper entries of J J^T, the 6 of J r and r^2 in f64 registers plus an integer inlier count;
//              then a butterfly over the wave, the 16 waves in order through LDS, and one partial per workgroup to scratch;
//   reduce     one workgroup: the partials are staged in LDS by all threads, then thread k sums row k in ascending workgroup order
//              (a first form summed straight from global memory: 172 us for 1024 partials, one dependent load per add).
// No floating-point atomics anywhere: for a given n_src the summation tree is fixed, so the sums are bit-reproducible.
#include "slr_device.hpp"

namespace slr {

constexpr int kIcpBlock = 1024;                // linearise: 16 waves, 4 per SIMD
constexpr unsigned kIcpMaxGroups = 256;        // linearise: at most one workgroup per CU; more points loop.  The reduce holds
                                               // all partials in LDS: 29 x 256 x 8 B = 58 KB
constexpr int kIcpNormBX = 64, kIcpNormBY = 4; // normals: one wave per row segment
// tests/np_icp_model.py (sum_depth) reads kIcpBlock and kIcpMaxGroups from this file and restates the summation tree below (grid-
// stride loop, butterfly over 64 lanes, the waves in order, the workgroups in order) to bound the rounding error of every sum.

unsigned icp_groups(size_t n_src)
{
    const size_t g = (n_src + kIcpBlock - 1) / kIcpBlock;
    return g < kIcpMaxGroups ? (unsigned)g : kIcpMaxGroups;
}
size_t icp_partial_bytes(size_t n_src)
{
    const size_t g = icp_groups(n_src);
    return (size_t)kIcpSums * 8 * (g ? g : 1);
}

__device__ __forceinline__ void icp_load(const float *__restrict__ xyz, size_t o, double p[3])
{
    p[0] = (double)xyz[3 * o]; p[1] = (double)xyz[3 * o + 1]; p[2] = (double)xyz[3 * o + 2];
}

// |a - c|^2 <= e2, summed x, y, z in that order (false for any NaN / inf)
__device__ __forceinline__ bool icp_near(const double a[3], const double c[3], double e2)
{
    const double dx = a[0] - c[0], dy = a[1] - c[1], dz = a[2] - c[2];
    return ((dx * dx + dy * dy) + dz * dz) <= e2;
}

__global__ __launch_bounds__(kIcpNormBX *kIcpNormBY) void icp_normals_kernel(const float *__restrict__ xyz,
                                                                             const uint8_t *__restrict__ has, int W, int H,
                                                                             double max_edge2, float *__restrict__ normals,
                                                                             uint8_t *__restrict__ nvalid)
{
    const int j = blockIdx.x * kIcpNormBX + threadIdx.x, i = blockIdx.y * kIcpNormBY + threadIdx.y;
    if (j >= W || i >= H) return;
    const size_t o = (size_t)i * W + j;
    float nf[3] = {0.f, 0.f, 0.f};
    uint8_t ok = 0;
    if (i >= 1 && i < H - 1 && j >= 1 && j < W - 1 && has[o] && has[o - 1] && has[o + 1] && has[o - W] && has[o + W]) {
        double c[3], l[3], r[3], u[3], d[3];
        icp_load(xyz, o, c); icp_load(xyz, o - 1, l); icp_load(xyz, o + 1, r); icp_load(xyz, o - W, u); icp_load(xyz, o + W, d);
        if (icp_near(l, c, max_edge2) && icp_near(r, c, max_edge2) && icp_near(u, c, max_edge2) && icp_near(d, c, max_edge2)) {
            const double a0 = r[0] - l[0], a1 = r[1] - l[1], a2 = r[2] - l[2];
            const double b0 = d[0] - u[0], b1 = d[1] - u[1], b2 = d[2] - u[2];
            double n0 = a1 * b2 - a2 * b1, n1 = a2 * b0 - a0 * b2, n2 = a0 * b1 - a1 * b0;
            const double m = __builtin_sqrt((n0 * n0 + n1 * n1) + n2 * n2);
            if (m != 0.0) {
                n0 = n0 / m; n1 = n1 / m; n2 = n2 / m;
                if ((n0 * c[0] + n1 * c[1]) + n2 * c[2] > 0.0) { n0 = -n0; n1 = -n1; n2 = -n2; }
                nf[0] = (float)n0; nf[1] = (float)n1; nf[2] = (float)n2;
                ok = 1;
            }
        }
    }
    normals[3 * o] = nf[0]; normals[3 * o + 1] = nf[1]; normals[3 * o + 2] = nf[2];
    nvalid[o] = ok;
}

// partials: [kIcpSums][groups] -- rows 0..27 f64 (21 upper J J^T, 6 J r, r^2), row 28 the inlier count as u64
__global__ __launch_bounds__(kIcpBlock) void icp_linearize_kernel(IcpLaunch a)
{
    double acc[kIcpSums - 1];
#pragma unroll
    for (int k = 0; k < kIcpSums - 1; k++) acc[k] = 0.0;
    unsigned cnt = 0;
    const size_t stride = (size_t)a.groups * kIcpBlock;
    for (size_t e = (size_t)blockIdx.x * kIcpBlock + threadIdx.x; e < a.n; e += stride) {
        if (a.src_has && !a.src_has[e]) continue;
        const float s0 = a.src[3 * e], s1 = a.src[3 * e + 1], s2 = a.src[3 * e + 2];
        if (!__builtin_isfinite(s0) || !__builtin_isfinite(s1) || !__builtin_isfinite(s2)) continue;
        double q[3];
#pragma unroll
        for (int r = 0; r < 3; r++)
            q[r] = ((a.T[4 * r] * (double)s0 + a.T[4 * r + 1] * (double)s1) + a.T[4 * r + 2] * (double)s2) + a.T[4 * r + 3];
        if (!(q[2] > 0.0)) continue;
        const double u = q[0] / q[2] * a.fx + a.cx, v = q[1] / q[2] * a.fy + a.cy;
        const double jf = __builtin_floor(u + 0.5), if_ = __builtin_floor(v + 0.5);
        if (!(jf >= 0.0 && jf < (double)a.W && if_ >= 0.0 && if_ < (double)a.H)) continue;   // doubles first: no int overflow
        const size_t o = (size_t)(int)if_ * a.W + (size_t)(int)jf;
        if (!a.dst_has[o] || !a.nvalid[o]) continue;
        const double dx = q[0] - (double)a.dst[3 * o], dy = q[1] - (double)a.dst[3 * o + 1], dz = q[2] - (double)a.dst[3 * o + 2];
        if (!(((dx * dx + dy * dy) + dz * dz) <= a.max_dist2)) continue;
        const double nx = (double)a.normals[3 * o], ny = (double)a.normals[3 * o + 1], nz = (double)a.normals[3 * o + 2];
        const double res = (nx * dx + ny * dy) + nz * dz;
        const double J[6] = {q[1] * nz - q[2] * ny, q[2] * nx - q[0] * nz, q[0] * ny - q[1] * nx, nx, ny, nz};
        int k = 0;
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = r; c < 6; c++) acc[k++] += J[r] * J[c];
#pragma unroll
        for (int r = 0; r < 6; r++) acc[21 + r] += J[r] * res;
        acc[27] += res * res;
        cnt++;
    }
    // the wave: a fixed butterfly
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < kIcpSums - 1; k++) acc[k] += __shfl_xor(acc[k], off, 64);
        cnt += __shfl_xor(cnt, off, 64);
    }
    __shared__ double wave_acc[kIcpBlock / 64][kIcpSums];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kIcpSums - 1; k++) wave_acc[wave][k] = acc[k];
        wave_acc[wave][kIcpSums - 1] = __longlong_as_double((long long)cnt);
    }
    __syncthreads();
    if (threadIdx.x < kIcpSums) {                      // the workgroup: its waves in order
        const int k = threadIdx.x;
        unsigned long long *row = reinterpret_cast<unsigned long long *>(a.partials) + (size_t)k * a.groups + blockIdx.x;
        if (k < kIcpSums - 1) {
            double s = wave_acc[0][k];
            for (int w = 1; w < kIcpBlock / 64; w++) s += wave_acc[w][k];
            *row = (unsigned long long)__double_as_longlong(s);
        } else {
            unsigned long long s = 0;
            for (int w = 0; w < kIcpBlock / 64; w++) s += (unsigned long long)__double_as_longlong(wave_acc[w][k]);
            *row = s;
        }
    }
}

__global__ __launch_bounds__(256) void icp_reduce_kernel(const double *__restrict__ partials, unsigned groups, double *__restrict__ out)
{
    __shared__ double stage[kIcpSums * kIcpMaxGroups];
    const unsigned total = kIcpSums * groups;
    for (unsigned x = threadIdx.x; x < total; x += 256) stage[x] = partials[x];
    __syncthreads();
    const int k = threadIdx.x;
    if (k >= kIcpSums) return;
    const double *row = stage + (size_t)k * groups;
    if (k < kIcpSums - 1) {
        double s = 0.0;
        for (unsigned w = 0; w < groups; w++) s += row[w];
        out[k] = s;
    } else {
        unsigned long long s = 0;
        for (unsigned w = 0; w < groups; w++) s += (unsigned long long)__double_as_longlong(row[w]);
        reinterpret_cast<unsigned long long *>(out)[k] = s;
    }
}

hipError_t launch_icp_normals(const float *xyz, const uint8_t *has, int W, int H, double max_edge, float *normals, uint8_t *nvalid,
                              hipStream_t s)
{
    const dim3 grid((unsigned)((W + kIcpNormBX - 1) / kIcpNormBX), (unsigned)((H + kIcpNormBY - 1) / kIcpNormBY));
    SLR_LAUNCH(icp_normals_kernel, grid, dim3(kIcpNormBX, kIcpNormBY), 0, s, xyz, has, W, H, max_edge * max_edge, normals, nvalid);
    return hipGetLastError();
}

hipError_t launch_icp_linearize(const IcpLaunch &L, hipStream_t s)
{
    if (L.groups) SLR_LAUNCH(icp_linearize_kernel, dim3(L.groups), dim3(kIcpBlock), 0, s, L);
    return hipGetLastError();
}

hipError_t launch_icp_reduce(const double *partials, unsigned groups, double *out, hipStream_t s)
{
    SLR_LAUNCH(icp_reduce_kernel, dim3(1), dim3(256), 0, s, partials, groups, out);
    return hipGetLastError();
}

}  // namespace slr
