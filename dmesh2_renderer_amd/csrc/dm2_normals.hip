// dm2_normals.hip -- Renderer.vertex_normals: area-weighted smooth normals of a triangle mesh and their gradient to the vertices,
// without float atomics (include/dm2_hip.h: dm2_vertex_normals).
//   k_face_normals     fn[f]  = (p1 - p0) x (p2 - p0), one 16-byte row per face (zeros for an invalid face)
//   k_vertex_normals   s[p]   = ((0 + fn[c0 / 3]) + fn[c1 / 3]) + ... over corners[offsets[p] .. offsets[p+1]), then s / |s| (or s)
//   k_face_normals_f64 the same cross product in double, one 32-byte row per face (backward, normalize only)
//   k_vertex_d         d[p]   = (g - n (n . g)) / len with n and len from the double rows (or d = g), one 16-byte row per vertex
//   k_corner_grads     cg[3 f + k] = the gradient face f sends to its corner k: D = (d_v0 + d_v1) + d_v2, c1 = e2 x D, c2 = D x e1,
//                      c0 = -(c1 + c2)
//   k_vertex_grads     dL/dverts[p] = the sum of cg over the vertex's corners, in the list's order
//
// The shape is Appendix B's store-and-sum: a pass over the faces stores every contribution once, in 16-byte rows at the address
// of its face (forward) or corner (backward), with consecutive lanes on consecutive rows; a pass over the vertices reads them
// back through the inverted index (offsets, corners) that Renderer.vertex_adjacency built, in the index's fixed order.  Every
// sum has one owner and one order: the results are a pure function of the inputs, and two calls give the same bits.  A lane
// owns a vertex and walks its list serially: meshes have valences of 4 to 8, where that is one short loop per lane; a fan of
// thousands of faces is correct and as slow as its longest list (load balancing of such fans is out of scope).
// -ffp-contract=off: the forward is a pure function of the written operation order (tests/normals_ref.py restates it).
//
// The backward does not take n and len of  d = (g - n (n . g)) / len  from the forward.  The forward's fp32 n carries the
// cancellation of its cross products: a face whose edges meet at a small angle a has a normal good to u / sin(a) only, and d
// inherits that error whole, which no term of the gradient's own sum covers (a fan of 2000 thin faces missed the per-element
// criterion by 2.2x that way).  So k_face_normals_f64 and k_vertex_d evaluate the same sums again in double, edges included,
// in the same list order; the forward's len only decides which vertices are zero, so forward and gradient agree on them.
#include <hip/hip_runtime.h>

#include "dm2_device_math.h"
#include "dm2_state.h"

namespace dm2 {

constexpr int VN_BLOCK = 256;

// the three vertices of face f; false: an invalid face (an id outside [0, P))
__device__ __forceinline__ bool vn_face(int f, int P, const float* __restrict__ verts, const int32_t* __restrict__ faces, int& i0,
                                        int& i1, int& i2, f3& p0, f3& p1, f3& p2) {
    i0 = faces[3 * (int64_t)f]; i1 = faces[3 * (int64_t)f + 1]; i2 = faces[3 * (int64_t)f + 2];
    if ((unsigned)i0 >= (unsigned)P || (unsigned)i1 >= (unsigned)P || (unsigned)i2 >= (unsigned)P) return false;
    p0 = {verts[3 * (int64_t)i0], verts[3 * (int64_t)i0 + 1], verts[3 * (int64_t)i0 + 2]};
    p1 = {verts[3 * (int64_t)i1], verts[3 * (int64_t)i1 + 1], verts[3 * (int64_t)i1 + 2]};
    p2 = {verts[3 * (int64_t)i2], verts[3 * (int64_t)i2 + 1], verts[3 * (int64_t)i2 + 2]};
    return true;
}

__global__ void __launch_bounds__(VN_BLOCK)
k_face_normals(int F, int P, const float* __restrict__ verts, const int32_t* __restrict__ faces, float4* __restrict__ fn) {
    const int64_t f = (int64_t)blockIdx.x * VN_BLOCK + threadIdx.x;
    if (f >= F) return;
    int i0, i1, i2;
    f3 p0, p1, p2, N = {0.0f, 0.0f, 0.0f};
    if (vn_face((int)f, P, verts, faces, i0, i1, i2, p0, p1, p2)) N = cross(p1 - p0, p2 - p0);
    fn[f] = make_float4(N.x, N.y, N.z, 0.0f);
}

// the list of vertex p, cut to the index's own extent whatever the offsets hold
__device__ __forceinline__ void vn_list(const int32_t* __restrict__ offsets, int64_t p, int F3, int& beg, int& end) {
    beg = min(max(offsets[p], 0), F3);
    end = min(max(offsets[p + 1], beg), F3);
}

// len > 0 and finite (false for NaN)
__device__ __forceinline__ bool vn_len_ok(float len) { return len > 0.0f && len < INFINITY; }

__global__ void __launch_bounds__(VN_BLOCK)
k_vertex_normals(int P, int F3, int normalize, const int32_t* __restrict__ offsets, const int32_t* __restrict__ corners,
                 const float4* __restrict__ fn, float* __restrict__ out, float* __restrict__ out_len) {
    const int64_t p = (int64_t)blockIdx.x * VN_BLOCK + threadIdx.x;
    if (p >= P) return;
    int beg, end;
    vn_list(offsets, p, F3, beg, end);
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int j = beg; j < end; j++) {
        const int c = corners[j];
        if ((unsigned)c >= (unsigned)F3) continue;                          // (not an index this library built)
        const float4 N = fn[c / 3];
        sx = sx + N.x; sy = sy + N.y; sz = sz + N.z;
    }
    const float len = sqrtf((sx * sx + sy * sy) + sz * sz);
    if (normalize) {
        const bool ok = vn_len_ok(len);
        sx = ok ? sx / len : 0.0f; sy = ok ? sy / len : 0.0f; sz = ok ? sz / len : 0.0f;
    }
    out[3 * p] = sx; out[3 * p + 1] = sy; out[3 * p + 2] = sz;
    if (out_len) out_len[p] = len;
}

// fn64: two double2 per face, (N.x, N.y) and (N.z, 0)
__global__ void __launch_bounds__(VN_BLOCK)
k_face_normals_f64(int F, int P, const float* __restrict__ verts, const int32_t* __restrict__ faces, double2* __restrict__ fn64) {
    const int64_t f = (int64_t)blockIdx.x * VN_BLOCK + threadIdx.x;
    if (f >= F) return;
    int i0, i1, i2;
    f3 p0, p1, p2;
    double nx = 0.0, ny = 0.0, nz = 0.0;
    if (vn_face((int)f, P, verts, faces, i0, i1, i2, p0, p1, p2)) {
        const double ax = (double)p1.x - (double)p0.x, ay = (double)p1.y - (double)p0.y, az = (double)p1.z - (double)p0.z;
        const double bx = (double)p2.x - (double)p0.x, by = (double)p2.y - (double)p0.y, bz = (double)p2.z - (double)p0.z;
        nx = ay * bz - az * by; ny = az * bx - ax * bz; nz = ax * by - ay * bx;
    }
    fn64[2 * f] = make_double2(nx, ny);
    fn64[2 * f + 1] = make_double2(nz, 0.0);
}

// normalize: n and len in double from fn64, summed in the list's order; a vertex the forward zeroed (lens) sends nothing.  Where
// the double sum has no direction although the forward's had one, the forward's n and len stand in.
__global__ void __launch_bounds__(VN_BLOCK)
k_vertex_d(int P, int F3, int normalize, const int32_t* __restrict__ offsets, const int32_t* __restrict__ corners,
           const double2* __restrict__ fn64, const float* __restrict__ normals, const float* __restrict__ lens,
           const float* __restrict__ g, float4* __restrict__ d) {
    const int64_t p = (int64_t)blockIdx.x * VN_BLOCK + threadIdx.x;
    if (p >= P) return;
    float dx = g[3 * p], dy = g[3 * p + 1], dz = g[3 * p + 2];
    if (normalize) {
        int beg, end;
        vn_list(offsets, p, F3, beg, end);
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int j = beg; j < end; j++) {
            const int c = corners[j];
            if ((unsigned)c >= (unsigned)F3) continue;
            const double2 a = fn64[2 * (int64_t)(c / 3)], b = fn64[2 * (int64_t)(c / 3) + 1];
            sx = sx + a.x; sy = sy + a.y; sz = sz + b.x;
        }
        double len = sqrt((sx * sx + sy * sy) + sz * sz);
        double nx, ny, nz;
        if (len > 0.0 && len < (double)INFINITY) {
            nx = sx / len; ny = sy / len; nz = sz / len;
        } else {
            len = (double)lens[p];
            nx = (double)normals[3 * p]; ny = (double)normals[3 * p + 1]; nz = (double)normals[3 * p + 2];
        }
        const double ng = (nx * (double)dx + ny * (double)dy) + nz * (double)dz;
        const bool ok = vn_len_ok(lens[p]);
        dx = ok ? (float)(((double)dx - nx * ng) / len) : 0.0f;
        dy = ok ? (float)(((double)dy - ny * ng) / len) : 0.0f;
        dz = ok ? (float)(((double)dz - nz * ng) / len) : 0.0f;
    }
    d[p] = make_float4(dx, dy, dz, 0.0f);
}

__global__ void __launch_bounds__(VN_BLOCK)
k_corner_grads(int F, int P, const float* __restrict__ verts, const int32_t* __restrict__ faces, const float4* __restrict__ d,
               float4* __restrict__ cg) {
    const int64_t f = (int64_t)blockIdx.x * VN_BLOCK + threadIdx.x;
    if (f >= F) return;
    int i0, i1, i2;
    f3 p0, p1, p2, c0 = {0.0f, 0.0f, 0.0f}, c1 = c0, c2 = c0;
    if (vn_face((int)f, P, verts, faces, i0, i1, i2, p0, p1, p2)) {
        const float4 d0 = d[i0], d1 = d[i1], d2 = d[i2];
        const f3 D = {(d0.x + d1.x) + d2.x, (d0.y + d1.y) + d2.y, (d0.z + d1.z) + d2.z};
        const f3 e1 = p1 - p0, e2 = p2 - p0;
        c1 = cross(e2, D);
        c2 = cross(D, e1);
        c0 = -(c1 + c2);
    }
    float4* row = cg + 3 * f;
    row[0] = make_float4(c0.x, c0.y, c0.z, 0.0f);
    row[1] = make_float4(c1.x, c1.y, c1.z, 0.0f);
    row[2] = make_float4(c2.x, c2.y, c2.z, 0.0f);
}

__global__ void __launch_bounds__(VN_BLOCK)
k_vertex_grads(int P, int F3, const int32_t* __restrict__ offsets, const int32_t* __restrict__ corners, const float4* __restrict__ cg,
               float* __restrict__ dverts) {
    const int64_t p = (int64_t)blockIdx.x * VN_BLOCK + threadIdx.x;
    if (p >= P) return;
    int beg, end;
    vn_list(offsets, p, F3, beg, end);
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int j = beg; j < end; j++) {
        const int c = corners[j];
        if ((unsigned)c >= (unsigned)F3) continue;
        const float4 r = cg[c];
        sx = sx + r.x; sy = sy + r.y; sz = sz + r.z;
    }
    dverts[3 * p] = sx; dverts[3 * p + 1] = sy; dverts[3 * p + 2] = sz;
}

static dim3 vn_grid(int64_t n) { return dim3((unsigned)((n + VN_BLOCK - 1) / VN_BLOCK)); }

size_t vertex_normals_scratch_bytes(int P, int F, int backward) {
    return backward ? ((size_t)P + 3 * (size_t)F) * sizeof(float4) : (size_t)F * sizeof(float4);
}

// P > 0; scratch: vertex_normals_scratch_bytes(P, F, 0) bytes, 16-byte aligned (unused when F == 0)
void launch_vertex_normals(int P, int F, int normalize, const float* verts, const int32_t* faces, const int32_t* offsets,
                           const int32_t* corners, void* scratch, float* out_normals, float* out_len, hipStream_t st) {
    float4* fn = reinterpret_cast<float4*>(scratch);
    if (F > 0) hipLaunchKernelGGL(k_face_normals, vn_grid(F), dim3(VN_BLOCK), 0, st, F, P, verts, faces, fn);
    hipLaunchKernelGGL(k_vertex_normals, vn_grid(P), dim3(VN_BLOCK), 0, st, P, 3 * F, normalize, offsets, corners, fn, out_normals,
                       out_len);
}

// P > 0; scratch: vertex_normals_scratch_bytes(P, F, 1) bytes, 16-byte aligned: P rows of d, then 3 F rows of corner terms (the
// double face normals, 2 F rows, lie in the corner terms' place until k_vertex_d has read them)
void launch_vertex_normals_backward(int P, int F, int normalize, const float* verts, const int32_t* faces, const int32_t* offsets,
                                    const int32_t* corners, const float* normals, const float* lens, const float* dL_dnormals,
                                    void* scratch, float* dL_dverts, hipStream_t st) {
    float4* d = reinterpret_cast<float4*>(scratch);
    float4* cg = d + P;
    if (F > 0) {
        double2* fn64 = reinterpret_cast<double2*>(cg);
        if (normalize) hipLaunchKernelGGL(k_face_normals_f64, vn_grid(F), dim3(VN_BLOCK), 0, st, F, P, verts, faces, fn64);
        hipLaunchKernelGGL(k_vertex_d, vn_grid(P), dim3(VN_BLOCK), 0, st, P, 3 * F, normalize, offsets, corners, fn64, normals, lens,
                           dL_dnormals, d);
        hipLaunchKernelGGL(k_corner_grads, vn_grid(F), dim3(VN_BLOCK), 0, st, F, P, verts, faces, d, cg);
    }
    hipLaunchKernelGGL(k_vertex_grads, vn_grid(P), dim3(VN_BLOCK), 0, st, P, 3 * F, offsets, corners, cg, dL_dverts);
}

}  // namespace dm2
