// Rays against the bounding-box mesh of the inpainting pipeline, for gfx950 (include/mvi_box_region.h): the reference's
// torchMesh.intersect (gs-simp/utils/bounding.py:62-121) splits the rays into chunks of 10 000 and evaluates ~30 PyTorch
// ops over [10000, F, 3] tensors per chunk; here one thread carries one ray through all faces in a single pass, keeping
// max_t, the smallest valid t with its first index and the first invalid index, and resolves the reference's sentinel rule
// (invalid faces take max_t + 1) at the end. The faces (v0, e1 = v1 - v0, e2 = v2 - v0) sit in LDS, read by every lane at
// one address (broadcast). The view-mask kernel builds each pixel's ray in registers (scene/helpers.py:107-140), so no ray
// tensor touches HBM.
//
// Bit parity with the reference: contraction is off for the whole file and every fused multiply-add is written out where
// PyTorch's CPU kernels fuse (cross product, vector norm, the [N,3] x [3,3] rotation of get_rays); the dot products are the
// reference's separate multiply and its (p0 + p1) + p2 sum. Division and sqrt are IEEE (hipcc's default for fp32).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mvi_box_region.h"
#include "../../include/mvi_raster.h"

#pragma clang fp contract(off)

namespace mvi {

static thread_local char g_berr[256] = "";

static int box_fail(int code, const char* msg) {
    snprintf(g_berr, sizeof(g_berr), "%s", msg);
    return code;
}

constexpr int kBrBlock = 256;     // rays (pixels) per block, one per thread
constexpr int kFaceChunk = 256;   // faces staged in LDS at a time (12 KiB); larger meshes loop over chunks

struct RayAcc {
    float maxt;   // max over all faces of t, invalid faces included
    float tmin;   // smallest t over the valid faces
    int imin;     // its first index, -1 = no valid face yet
    int iinv;     // first invalid face, -1 = none yet
};

struct RayOut {
    float t;      // int_t (0 where !cond)
    int ind;      // t_ind
    bool cond;
};

__device__ __forceinline__ void cross_fma(float ax, float ay, float az, float bx, float by, float bz, float& cx, float& cy,
                                          float& cz) {
    cx = fmaf(ay, bz, -(az * by));
    cy = fmaf(az, bx, -(ax * bz));
    cz = fmaf(ax, by, -(ay * bx));
}

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    const float p0 = ax * bx, p1 = ay * by, p2 = az * bz;
    return (p0 + p1) + p2;
}

// F.normalize(d, p=2, dim=-1): d / max(|d|, 1e-12), the norm as fma(z, z, fma(y, y, x * x))
__device__ __forceinline__ void normalize3(float& x, float& y, float& z) {
    const float n = sqrtf(fmaf(z, z, fmaf(y, y, x * x)));
    const float den = n < 1e-12f ? 1e-12f : n;
    x = x / den;
    y = y / den;
    z = z / den;
}

// Stages faces [base, base + nf) of f_v into LDS as three float4 per face: (v0, e1x) (e1yz, e2xy) (e2z, -, -, -).
__device__ __forceinline__ void stage_faces(const float* __restrict__ f_v, int base, int nf, float4* s_f) {
    for (int k = threadIdx.x; k < nf; k += blockDim.x) {
        const float* p = f_v + 9 * (size_t)(base + k);
        const float v0x = p[0], v0y = p[1], v0z = p[2];
        const float e1x = p[3] - v0x, e1y = p[4] - v0y, e1z = p[5] - v0z;
        const float e2x = p[6] - v0x, e2y = p[7] - v0y, e2z = p[8] - v0z;
        s_f[3 * k + 0] = make_float4(v0x, v0y, v0z, e1x);
        s_f[3 * k + 1] = make_float4(e1y, e1z, e2x, e2y);
        s_f[3 * k + 2] = make_float4(e2z, 0.f, 0.f, 0.f);
    }
}

__device__ __forceinline__ void visit_faces(const float4* s_f, int nf, int base, float ox, float oy, float oz, float dx,
                                            float dy, float dz, RayAcc& r) {
    const float eps = 1e-8f;
    for (int k = 0; k < nf; ++k) {
        const float4 f0 = s_f[3 * k], f1 = s_f[3 * k + 1], f2 = s_f[3 * k + 2];
        const float e1x = f0.w, e1y = f1.x, e1z = f1.y, e2x = f1.z, e2y = f1.w, e2z = f2.x;
        float hx, hy, hz;
        cross_fma(dx, dy, dz, e2x, e2y, e2z, hx, hy, hz);
        const float a = dot3(e1x, e1y, e1z, hx, hy, hz);
        const float f = 1.f / (a + eps);
        const float sx = ox - f0.x, sy = oy - f0.y, sz = oz - f0.z;
        const float u = f * dot3(sx, sy, sz, hx, hy, hz);
        float qx, qy, qz;
        cross_fma(sx, sy, sz, e1x, e1y, e1z, qx, qy, qz);
        const float v = f * dot3(dx, dy, dz, qx, qy, qz);
        const float t = f * dot3(e2x, e2y, e2z, qx, qy, qz);
        const bool bad = (a > -eps && a < eps) || u < 0.f || u > 1.f || v < 0.f || (u + v) > 1.f || t < eps;
        r.maxt = t > r.maxt ? t : r.maxt;
        if (!bad && (r.imin < 0 || t < r.tmin)) {
            r.tmin = t;
            r.imin = base + k;
        }
        if (bad && r.iinv < 0) r.iinv = base + k;
    }
}

// torch.min over (invalid ? max_t + 1 : t) with the first index of the minimum, then the reference's cond
__device__ __forceinline__ RayOut resolve(const RayAcc& r) {
    const float m1 = r.maxt + 1.f;
    float mn;
    int idx;
    if (r.imin >= 0 && (r.iinv < 0 || r.tmin < m1 || (r.tmin == m1 && r.imin < r.iinv))) {
        mn = r.tmin;
        idx = r.imin;
    } else {
        mn = m1;
        idx = r.iinv;
    }
    RayOut o;
    o.cond = (m1 - mn) > 0.f;
    o.t = o.cond ? mn : 0.f;
    o.ind = idx;
    return o;
}

__device__ __forceinline__ RayAcc ray_acc_init() {
    RayAcc r;
    r.maxt = -INFINITY;
    r.tmin = 0.f;
    r.imin = -1;
    r.iinv = -1;
    return r;
}

__global__ __launch_bounds__(kBrBlock) void mesh_intersect_kernel(const float* __restrict__ o, const float* __restrict__ d,
                                                                  int64_t n, const float* __restrict__ f_v, int F,
                                                                  float* __restrict__ int_p, float* __restrict__ int_t,
                                                                  int64_t* __restrict__ t_ind, uint8_t* __restrict__ cond) {
    __shared__ float4 s_f[3 * kFaceChunk];
    const int64_t i = (int64_t)blockIdx.x * kBrBlock + threadIdx.x;
    const bool live = i < n;
    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 1.f;
    if (live) {
        ox = o[3 * i]; oy = o[3 * i + 1]; oz = o[3 * i + 2];
        dx = d[3 * i]; dy = d[3 * i + 1]; dz = d[3 * i + 2];
    }
    normalize3(dx, dy, dz);
    RayAcc r = ray_acc_init();
    for (int base = 0; base < F; base += kFaceChunk) {
        const int nf = min(kFaceChunk, F - base);
        __syncthreads();
        stage_faces(f_v, base, nf, s_f);
        __syncthreads();
        visit_faces(s_f, nf, base, ox, oy, oz, dx, dy, dz, r);
    }
    if (!live) return;
    const RayOut h = resolve(r);
    int_t[i] = h.t;
    t_ind[i] = h.ind;
    cond[i] = h.cond ? 1 : 0;
    int_p[3 * i] = h.cond ? ox + h.t * dx : 0.f;
    int_p[3 * i + 1] = h.cond ? oy + h.t * dy : 0.f;
    int_p[3 * i + 2] = h.cond ? oz + h.t * dz : 0.f;
}

// del.py: inside = (int_t(+x) > 0) & (int_t(-x) > 0). (1, 0, 0) is its own normalisation.
__global__ __launch_bounds__(kBrBlock) void mesh_points_inside_kernel(const float* __restrict__ xyz, int64_t N,
                                                                      const float* __restrict__ f_v, int F,
                                                                      uint8_t* __restrict__ inside) {
    __shared__ float4 s_f[3 * kFaceChunk];
    const int64_t i = (int64_t)blockIdx.x * kBrBlock + threadIdx.x;
    const bool live = i < N;
    float ox = 0.f, oy = 0.f, oz = 0.f;
    if (live) {
        ox = xyz[3 * i]; oy = xyz[3 * i + 1]; oz = xyz[3 * i + 2];
    }
    RayAcc rp = ray_acc_init(), rn = ray_acc_init();
    for (int base = 0; base < F; base += kFaceChunk) {
        const int nf = min(kFaceChunk, F - base);
        __syncthreads();
        stage_faces(f_v, base, nf, s_f);
        __syncthreads();
        visit_faces(s_f, nf, base, ox, oy, oz, 1.f, 0.f, 0.f, rp);
        visit_faces(s_f, nf, base, ox, oy, oz, -1.f, 0.f, 0.f, rn);
    }
    if (!live) return;
    inside[i] = (resolve(rp).t > 0.f && resolve(rn).t > 0.f) ? 1 : 0;
}

__global__ __launch_bounds__(kBrBlock) void mesh_view_masks_kernel(const float* __restrict__ c2w, const float* __restrict__ fxs,
                                                                   const float* __restrict__ fys, int H, int W,
                                                                   const float* __restrict__ f_v, int F,
                                                                   const float* __restrict__ depth,
                                                                   const float* __restrict__ render, float* __restrict__ mask,
                                                                   float* __restrict__ masked, float* __restrict__ disparity) {
    __shared__ float4 s_f[3 * kFaceChunk];
    const int view = blockIdx.y;
    const int64_t HW = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * kBrBlock + threadIdx.x;
    const bool live = p < HW;
    const float* M = c2w + 16 * (size_t)view;
    const float fx = fxs[view], fy = fys[view];
    const int px = live ? (int)(p % W) : 0, py = live ? (int)(p / W) : 0;
    // get_rays: i = linspace(0, W - 1, W) + 0.5, xs = (i - W // 2) / fx, ys likewise, zs = 1; rays_d = dirs @ R^T
    const float xs = (((float)px + 0.5f) - (float)(W / 2)) / fx;
    const float ys = (((float)py + 0.5f) - (float)(H / 2)) / fy;
    float dx = fmaf(1.f, M[2], fmaf(ys, M[1], xs * M[0]));
    float dy = fmaf(1.f, M[6], fmaf(ys, M[5], xs * M[4]));
    float dz = fmaf(1.f, M[10], fmaf(ys, M[9], xs * M[8]));
    const float ox = M[3], oy = M[7], oz = M[11];
    normalize3(dx, dy, dz);
    RayAcc r = ray_acc_init();
    for (int base = 0; base < F; base += kFaceChunk) {
        const int nf = min(kFaceChunk, F - base);
        __syncthreads();
        stage_faces(f_v, base, nf, s_f);
        __syncthreads();
        visit_faces(s_f, nf, base, ox, oy, oz, dx, dy, dz, r);
    }
    if (!live) return;
    const float t = resolve(r).t;
    const size_t q = (size_t)view * HW + p;
    const float z = depth[q];
    const float m = (t > 0.f && (t < z || z == 15.f)) ? 1.f : 0.f;
    mask[q] = m;
    if (masked) {
        const float keep = 1.f - m;
        const size_t c0 = (size_t)view * 3 * HW + p;
#pragma unroll
        for (int c = 0; c < 3; ++c) masked[c0 + c * HW] = render[c0 + c * HW] * keep + m;
    }
    if (disparity) disparity[q] = 1.f / (z < 1e-3f ? 1e-3f : z);
}

static int launch_status(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_berr, sizeof(g_berr), "%s: %s", what, hipGetErrorString(e));
        return MVI_EHIP;
    }
    return MVI_OK;
}

static int check_mesh(const float* f_v, int32_t F) {
    if (F < 1) return box_fail(MVI_EINVAL, "the mesh needs at least one face (F >= 1)");
    if (!f_v) return box_fail(MVI_EINVAL, "f_v is NULL");
    return MVI_OK;
}

}  // namespace mvi

using namespace mvi;

extern "C" int mvi_mesh_intersect(const float* o, const float* d, int64_t n, const float* f_v, int32_t F, float* int_p,
                                  float* int_t, int64_t* t_ind, uint8_t* cond, void* stream) {
    if (int rc = check_mesh(f_v, F)) return rc;
    if (n < 0) return box_fail(MVI_EINVAL, "n < 0");
    if (n == 0) return MVI_OK;
    if (!o || !d || !int_p || !int_t || !t_ind || !cond) return box_fail(MVI_EINVAL, "mvi_mesh_intersect: NULL array");
    const int64_t blocks = (n + kBrBlock - 1) / kBrBlock;
    if (blocks > 0x7fffffff) return box_fail(MVI_EINVAL, "mvi_mesh_intersect: too many rays");
    hipLaunchKernelGGL(mesh_intersect_kernel, dim3((unsigned)blocks), dim3(kBrBlock), 0, (hipStream_t)stream, o, d, n, f_v, F,
                       int_p, int_t, t_ind, cond);
    return launch_status("mesh_intersect_kernel");
}

extern "C" int mvi_mesh_points_inside(const float* xyz, int64_t N, const float* f_v, int32_t F, uint8_t* inside, void* stream) {
    if (int rc = check_mesh(f_v, F)) return rc;
    if (N < 0) return box_fail(MVI_EINVAL, "N < 0");
    if (N == 0) return MVI_OK;
    if (!xyz || !inside) return box_fail(MVI_EINVAL, "mvi_mesh_points_inside: NULL array");
    const int64_t blocks = (N + kBrBlock - 1) / kBrBlock;
    if (blocks > 0x7fffffff) return box_fail(MVI_EINVAL, "mvi_mesh_points_inside: too many points");
    hipLaunchKernelGGL(mesh_points_inside_kernel, dim3((unsigned)blocks), dim3(kBrBlock), 0, (hipStream_t)stream, xyz, N, f_v, F,
                       inside);
    return launch_status("mesh_points_inside_kernel");
}

extern "C" int mvi_mesh_view_masks(const float* c2w, const float* fx, const float* fy, int32_t V, int32_t H, int32_t W,
                                   const float* f_v, int32_t F, const float* depth, const float* render, float* mask,
                                   float* masked, float* disparity, void* stream) {
    if (int rc = check_mesh(f_v, F)) return rc;
    if (V < 0 || H < 0 || W < 0) return box_fail(MVI_EINVAL, "negative view count or size");
    if (V > 65535) return box_fail(MVI_EINVAL, "at most 65535 views per call");
    if ((render == nullptr) != (masked == nullptr)) return box_fail(MVI_EINVAL, "render and masked go together");
    if ((int64_t)V * H * W == 0) return MVI_OK;
    if (!c2w || !fx || !fy || !depth || !mask) return box_fail(MVI_EINVAL, "mvi_mesh_view_masks: NULL array");
    const int64_t blocks = ((int64_t)H * W + kBrBlock - 1) / kBrBlock;
    if (blocks > 0x7fffffff) return box_fail(MVI_EINVAL, "mvi_mesh_view_masks: view too large");
    hipLaunchKernelGGL(mesh_view_masks_kernel, dim3((unsigned)blocks, (unsigned)V), dim3(kBrBlock), 0, (hipStream_t)stream, c2w,
                       fx, fy, H, W, f_v, F, depth, render, mask, masked, disparity);
    return launch_status("mesh_view_masks_kernel");
}

extern "C" const char* mvi_box_region_last_error(void) { return g_berr; }
