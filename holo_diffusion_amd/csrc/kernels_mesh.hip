// kernels_mesh.hip — a voxel grid leaves the library as geometry: the density of the rendered field on a regular
// lattice, and surface nets on a scalar lattice field (include/holo_abi.h: holo_density_lattice, holo_surface_count,
// holo_surface_emit).
//
// Surface nets, as pinned in the header: one vertex per lattice cell the surface crosses (the mean of the crossing points
// of the cell's sign-changing edges), one quad per lattice edge whose endpoints lie on different sides.  Four passes:
//   1 classify   one thread per lattice POINT p = (i, j, k): is the cell whose lowest corner is p active (0 / 1), and how
//                many of p's three edges (+x, +y, +z) change side (0..3) - both in one 64-bit word, cell flag in the low
//                half, quads in the high half
//   2 scan       exclusive scan of the m^3 + 1 words (block scans of 256, recursively over the block totals): the low half
//                of word p is then the vertex index of cell p, the high half the index of p's first quad, word m^3 the totals
//   3 vertices   one thread per lattice point, active cells recompute their eight corners and write their vertex
//   4 triangles  one thread per lattice point, every sign-changing edge looks up the vertex indices of its four cells
// Every index comes from the scan: no atomics anywhere, the output order is fixed (vertices by cell linear index, faces by
// (lattice point linear index, axis)).  All linear indices are 64-bit (m = 1024: 2^30 points).  The arithmetic is float32
// with contraction off, so that tests/support/surface_nets_ref.py restates it bit for bit.  Non-finite field values are
// out of scope.  This first form reads the eight corners of a cell through the cache; an LDS-tiled form is a later change.
#include <math.h>

#include "holo_common.h"
#include "holo_kernels.h"

namespace holo {
namespace {

constexpr int SCAN_B = 256;  // elements (= threads) of one block scan

__device__ __forceinline__ float leaky02(float v) { return fmaxf(v, 0.2f * v); }
// x / h for a wave-uniform h, rh = 1 / h: the form eval_point uses (kernels_render.hip, div_uniform), repeated here so that
// the lattice and holo_implicit_eval see the same local coordinate for the same point
__device__ __forceinline__ float div_uniform(float x, float h, float rh) {
  const float q = x * rh;
  return fmaf(fmaf(-q, h, x), rh, q);
}

// (i, j, k) of a lattice point's linear index.  The index itself is 64-bit wherever it addresses memory; m <= 1024 keeps it
// below 2^30 + 1, so it is taken apart with two 32-bit divisions (a 64-bit division costs several times as much).
__device__ __forceinline__ void lattice_ijk(int64_t idx, int m, int& i, int& j, int& k) {
  const uint32_t p = (uint32_t)idx, um = (uint32_t)m;
  const uint32_t row = p / um, plane = row / um;
  i = (int)(p - row * um);
  j = (int)(row - plane * um);
  k = (int)plane;
}

// world coordinate of lattice index i (the ONE pinned form, also of the vertices: (index + local) * spacing - h)
__device__ __forceinline__ float lattice_coord(float index, float spacing, float half_extent) {
#pragma clang fp contract(off)
  return index * spacing - half_extent;
}

// density = LeakyReLU(trilerp(S)(p) + b_dens) at the m^3 lattice points; S [R][R][R] from density_field_kernel.  The local
// coordinate, the voxel index and the zero weight of corners outside the grid are eval_point's.
__global__ __launch_bounds__(256) void density_lattice_kernel(const float* __restrict__ S, int R, float half_extent,
                                                              float b_dens, int m, float spacing, int64_t n,
                                                              float* __restrict__ field) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  int i, j, k;
  lattice_ijk(idx, m, i, j, k);
  const float px = lattice_coord((float)i, spacing, half_extent), py = lattice_coord((float)j, spacing, half_extent),
              pz = lattice_coord((float)k, spacing, half_extent);
  const float Rm1 = (float)(R - 1);
  const float rh = holo_rcp_exact(half_extent);
  const float lx = div_uniform(px, half_extent, rh), ly = div_uniform(py, half_extent, rh), lz = div_uniform(pz, half_extent, rh);
  const float ix = ((lx + 1.f) * 0.5f) * Rm1, iy = ((ly + 1.f) * 0.5f) * Rm1, iz = ((lz + 1.f) * 0.5f) * Rm1;
  const float fx0 = floorf(ix), fy0 = floorf(iy), fz0 = floorf(iz);
  const float wx[2] = {(fx0 >= 0.f && fx0 <= Rm1) ? (fx0 + 1.f) - ix : 0.f, (fx0 >= -1.f && fx0 <= Rm1 - 1.f) ? ix - fx0 : 0.f};
  const float wy[2] = {(fy0 >= 0.f && fy0 <= Rm1) ? (fy0 + 1.f) - iy : 0.f, (fy0 >= -1.f && fy0 <= Rm1 - 1.f) ? iy - fy0 : 0.f};
  const float wz[2] = {(fz0 >= 0.f && fz0 <= Rm1) ? (fz0 + 1.f) - iz : 0.f, (fz0 >= -1.f && fz0 <= Rm1 - 1.f) ? iz - fz0 : 0.f};
  const int x0 = (int)fminf(fmaxf(fx0, -1.f), Rm1), y0 = (int)fminf(fmaxf(fy0, -1.f), Rm1), z0 = (int)fminf(fmaxf(fz0, -1.f), Rm1);
  const int xs[2] = {max(x0, 0), min(x0 + 1, R - 1)};
  const int ys[2] = {max(y0, 0), min(y0 + 1, R - 1)};
  const int zs[2] = {max(z0, 0), min(z0 + 1, R - 1)};
  float z = b_dens;
#pragma unroll
  for (int corner = 0; corner < 8; ++corner) {
    const int dx = corner & 1, dy = (corner >> 1) & 1, dz = corner >> 2;
    z = fmaf((wx[dx] * wy[dy]) * wz[dz], S[((int64_t)zs[dz] * R + ys[dy]) * R + xs[dx]], z);
  }
  field[idx] = leaky02(z);
}

// f' of lattice point (x, y, z): the field, except on the outermost layer, where f' = level - |field - level| (never
// inside, so every mesh is closed)
__device__ __forceinline__ float field_value(const float* __restrict__ field, int m, int x, int y, int z, float level) {
#pragma clang fp contract(off)
  const float f = field[((int64_t)z * m + y) * m + x];
  const bool edge = x == 0 || y == 0 || z == 0 || x == m - 1 || y == m - 1 || z == m - 1;
  return edge ? level - fabsf(f - level) : f;
}

// pass 1 (file header).  Corners past the lattice are clamped onto the point itself: they then agree with it, so a
// point of the last layer has no cell and its missing edges no quads.
__global__ __launch_bounds__(256) void surface_classify_kernel(const float* __restrict__ field, int m, float level, int64_t n,
                                                               unsigned long long* __restrict__ words) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx > n) return;
  if (idx == n) {  // the slot whose scan is the totals
    words[n] = 0ull;
    return;
  }
  int i, j, k;
  lattice_ijk(idx, m, i, j, k);
  const int i1 = min(i + 1, m - 1), j1 = min(j + 1, m - 1), k1 = min(k + 1, m - 1);
  bool in[8];
#pragma unroll
  for (int c = 0; c < 8; ++c)
    in[c] = field_value(field, m, (c & 1) ? i1 : i, (c & 2) ? j1 : j, (c & 4) ? k1 : k, level) > level;
  int n_in = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) n_in += in[c] ? 1 : 0;
  const bool cell = i < m - 1 && j < m - 1 && k < m - 1 && n_in != 0 && n_in != 8;
  const unsigned long long quads = (in[0] != in[1] ? 1 : 0) + (in[0] != in[2] ? 1 : 0) + (in[0] != in[4] ? 1 : 0);
  words[idx] = (quads << 32) | (cell ? 1ull : 0ull);
}

// pass 2: exclusive scan of one block's SCAN_B words in place; the block's total goes to sums[block] (null: single block)
__global__ __launch_bounds__(SCAN_B) void surface_scan_kernel(unsigned long long* __restrict__ data, int64_t n,
                                                              unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long s_scan[SCAN_B];
  const int tid = threadIdx.x;
  const int64_t idx = (int64_t)blockIdx.x * SCAN_B + tid;
  const unsigned long long v = idx < n ? data[idx] : 0ull;
  s_scan[tid] = v;
  __syncthreads();
  for (int off = 1; off < SCAN_B; off <<= 1) {
    const unsigned long long t = tid >= off ? s_scan[tid - off] : 0ull;
    __syncthreads();
    s_scan[tid] += t;
    __syncthreads();
  }
  if (idx < n) data[idx] = s_scan[tid] - v;
  if (sums && tid == SCAN_B - 1) sums[blockIdx.x] = s_scan[tid];
}

// ... and the scanned block totals added back to every word of their block
__global__ __launch_bounds__(SCAN_B) void surface_scan_add_kernel(unsigned long long* __restrict__ data, int64_t n,
                                                                  const unsigned long long* __restrict__ sums) {
  const int64_t idx = (int64_t)blockIdx.x * SCAN_B + threadIdx.x;
  if (idx < n) data[idx] += sums[blockIdx.x];
}

// (vertices, triangles) from the totals word
__global__ __launch_bounds__(64) void surface_totals_kernel(const unsigned long long* __restrict__ total,
                                                            int64_t* __restrict__ counts) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const unsigned long long w = *total;
  counts[0] = (int64_t)(w & 0xffffffffull);
  counts[1] = 2 * (int64_t)(w >> 32);
}

// pass 3.  status[0] = 1 when a vertex did not fit verts_capacity (nothing is written past it).
__global__ __launch_bounds__(256) void surface_vertices_kernel(const float* __restrict__ field, int m, float level,
                                                               float half_extent, float spacing, int64_t n,
                                                               const unsigned long long* __restrict__ words,
                                                               float* __restrict__ verts, int64_t verts_capacity,
                                                               int* __restrict__ status) {
#pragma clang fp contract(off)
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const unsigned long long w = words[idx];
  if ((uint32_t)words[idx + 1] == (uint32_t)w) return;  // no vertex in this cell
  const int64_t vid = (int64_t)(uint32_t)w;
  if (vid >= verts_capacity) {
    status[0] = 1;
    return;
  }
  int i, j, k;
  lattice_ijk(idx, m, i, j, k);
  if (i >= m - 1 || j >= m - 1 || k >= m - 1) return;  // (words that are not this field's: no read past the lattice)
  float f[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) f[c] = field_value(field, m, i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2), level);
  // crossing points in the fixed order: axis x, y, z; within an axis (u, v) = (0,0), (0,1), (1,0), (1,1) over the axes
  // (axis + 1) % 3 and (axis + 2) % 3
  float acc[3] = {0.f, 0.f, 0.f};
  int count = 0;
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
#pragma unroll
    for (int uv = 0; uv < 4; ++uv) {
      const int au = (ax + 1) % 3, av = (ax + 2) % 3, u = uv >> 1, v = uv & 1;
      const int ca = (u << au) | (v << av), cb = ca | (1 << ax);
      const float fa = f[ca], fb = f[cb];
      if ((fa > level) == (fb > level)) continue;
      const float t = (fa - level) / (fa - fb);
      acc[ax] += t;
      acc[au] += (float)u;
      acc[av] += (float)v;
      ++count;
    }
  }
  if (count == 0) return;  // (only with words that are not this field's)
  const float cf = (float)count;
  verts[vid * 3 + 0] = lattice_coord((float)i + acc[0] / cf, spacing, half_extent);
  verts[vid * 3 + 1] = lattice_coord((float)j + acc[1] / cf, spacing, half_extent);
  verts[vid * 3 + 2] = lattice_coord((float)k + acc[2] / cf, spacing, half_extent);
}

// pass 4.  status[1] = 1 when a quad's two triangles did not fit tris_capacity (nothing is written past it).
__global__ __launch_bounds__(256) void surface_triangles_kernel(const float* __restrict__ field, int m, float level, int64_t n,
                                                                const unsigned long long* __restrict__ words,
                                                                int32_t* __restrict__ faces, int64_t tris_capacity,
                                                                int* __restrict__ status) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const unsigned long long w = words[idx];
  int64_t quad = (int64_t)(w >> 32);
  if ((int64_t)(words[idx + 1] >> 32) == quad) return;  // none of this point's edges changes side
  int p[3];
  lattice_ijk(idx, m, p[0], p[1], p[2]);
  const bool in0 = field_value(field, m, p[0], p[1], p[2], level) > level;
  const int64_t stride[3] = {1, m, (int64_t)m * m};
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    const int au = (ax + 1) % 3, av = (ax + 2) % 3;
    if (p[ax] + 1 >= m) continue;
    int q[3] = {p[0], p[1], p[2]};
    q[ax] += 1;
    if ((field_value(field, m, q[0], q[1], q[2], level) > level) == in0) continue;
    // the boundary rule puts the four cells around the edge in range; checked all the same (words of another field)
    if (p[au] < 1 || p[av] < 1) continue;
    const int64_t c00 = idx - stride[au] - stride[av];
    int32_t v[4] = {(int32_t)(uint32_t)words[c00], (int32_t)(uint32_t)words[c00 + stride[au]],
                    (int32_t)(uint32_t)words[idx], (int32_t)(uint32_t)words[c00 + stride[av]]};
    if (!in0) {  // normals from inside to outside
      int32_t t = v[0];
      v[0] = v[3];
      v[3] = t;
      t = v[1];
      v[1] = v[2];
      v[2] = t;
    }
    const int64_t t0 = 2 * quad;
    ++quad;
    if (t0 + 2 > tris_capacity) {
      status[1] = 1;
      continue;
    }
    int32_t* o = faces + t0 * 3;
    o[0] = v[0], o[1] = v[1], o[2] = v[2];
    o[3] = v[0], o[4] = v[2], o[5] = v[3];
  }
}

inline int64_t lattice_points(int m) { return (int64_t)m * m * m; }
// workspace: status (two ints) | words [m^3 + 1] | block totals of every scan level
constexpr size_t STATUS_BYTES = 256;
inline size_t words_bytes(int m) { return align256((size_t)(lattice_points(m) + 1) * sizeof(unsigned long long)); }

// exclusive scan of data[0..n) in place; `sums` has room for the block totals of this and every further level
void scan_launch(unsigned long long* data, int64_t n, unsigned long long* sums, void* stream) {
  const int64_t nb = cdiv(n, SCAN_B);
  if (nb == 1) {
    HOLO_LAUNCH(surface_scan_kernel, dim3(1), dim3(SCAN_B), stream, data, n, (unsigned long long*)nullptr);
    return;
  }
  HOLO_LAUNCH(surface_scan_kernel, dim3((unsigned)nb), dim3(SCAN_B), stream, data, n, sums);
  scan_launch(sums, nb, sums + align256((size_t)nb * sizeof(unsigned long long)) / sizeof(unsigned long long), stream);
  HOLO_LAUNCH(surface_scan_add_kernel, dim3((unsigned)nb), dim3(SCAN_B), stream, data, n, (const unsigned long long*)sums);
}

}  // namespace

int density_lattice_launch(const float* S, int R, float half_extent, float b_dens, int m, float* field, void* stream) {
  const int64_t n = lattice_points(m);
  HOLO_LAUNCH(density_lattice_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), stream, S, R, half_extent, b_dens, m,
              lattice_spacing(half_extent, m), n, field);
  return 0;
}

size_t surface_workspace_bytes(int m) {
  size_t b = STATUS_BYTES + words_bytes(m);
  for (int64_t nb = cdiv(lattice_points(m) + 1, SCAN_B); nb > 1; nb = cdiv(nb, SCAN_B))
    b += align256((size_t)nb * sizeof(unsigned long long));
  return b + 256;  // (the last level's totals: one block, never written)
}

int surface_count_launch(const float* field, int m, float level, int64_t* counts, void* workspace, void* stream) {
  const int64_t n = lattice_points(m);
  unsigned long long* words = (unsigned long long*)((char*)workspace + STATUS_BYTES);
  HOLO_LAUNCH(surface_classify_kernel, dim3((unsigned)cdiv(n + 1, 256)), dim3(256), stream, field, m, level, n, words);
  scan_launch(words, n + 1, (unsigned long long*)((char*)workspace + STATUS_BYTES + words_bytes(m)), stream);
  HOLO_LAUNCH(surface_totals_kernel, dim3(1), dim3(64), stream, (const unsigned long long*)(words + n), counts);
  return 0;
}

int surface_emit_launch(const float* field, int m, float level, float half_extent, float* verts, int64_t verts_capacity,
                        int32_t* faces, int64_t tris_capacity, void* workspace, void* stream) {
  const int64_t n = lattice_points(m);
  int* status = (int*)workspace;
  const unsigned long long* words = (const unsigned long long*)((char*)workspace + STATUS_BYTES);
  HIP_TRY(hipMemsetAsync(status, 0, 2 * sizeof(int), (hipStream_t)stream));
  const dim3 grid((unsigned)cdiv(n, 256));
  if (verts)
    HOLO_LAUNCH(surface_vertices_kernel, grid, dim3(256), stream, field, m, level, half_extent, lattice_spacing(half_extent, m),
                n, words, verts, verts_capacity, status);
  if (faces)
    HOLO_LAUNCH(surface_triangles_kernel, grid, dim3(256), stream, field, m, level, n, words, faces, tris_capacity, status);
  return 0;
}

}  // namespace holo
