// mesh_exec.cpp — host side of the surface extraction (kernels_mesh.hip): argument checks and the two launches of
// include/holo_abi.h's holo_surface_count / holo_surface_emit.  (holo_density_lattice needs the renderer's folded density
// row and lives with it in render_exec.cpp.)
#include <math.h>

#include "../../include/holo_abi.h"
#include "holo_common.h"
#include "holo_kernels.h"

using namespace holo;

// the checks both entries share; 0 or the error code (message set)
static int surface_args(const char* entry, const HoloCtx* ctx, const float* field, int m, float level, const void* workspace,
                        size_t workspace_bytes) {
  if (!ctx || !field || !workspace) {
    set_error("%s: null argument", entry);
    return HOLO_E_INVALID;
  }
  if (m < 2 || m > 1024) {
    set_error("%s: the lattice has 2 <= m <= 1024 points per axis (got %d)", entry, m);
    return HOLO_E_INVALID;
  }
  if (!isfinite(level)) {
    set_error("%s: level must be finite", entry);
    return HOLO_E_INVALID;
  }
  if (workspace_bytes < surface_workspace_bytes(m)) {
    set_error("%s: workspace too small (holo_surface_workspace_bytes)", entry);
    return HOLO_E_WORKSPACE;
  }
  return 0;
}

extern "C" {

size_t holo_surface_workspace_bytes(int m) { return (m < 2 || m > 1024) ? 0 : surface_workspace_bytes(m); }

int holo_surface_count(HoloCtx* ctx, const float* field, int m, float level, int64_t* counts_dev, void* workspace,
                       size_t workspace_bytes, void* stream) {
  if (const int rc = surface_args("holo_surface_count", ctx, field, m, level, workspace, workspace_bytes)) return rc;
  if (!counts_dev) {
    set_error("holo_surface_count: null argument");
    return HOLO_E_INVALID;
  }
  return surface_count_launch(field, m, level, counts_dev, workspace, stream);
}

int holo_surface_emit(HoloCtx* ctx, const float* field, int m, float level, float half_extent, float* verts,
                      int64_t verts_capacity, int32_t* faces, int64_t tris_capacity, void* workspace, size_t workspace_bytes,
                      void* stream) {
  if (const int rc = surface_args("holo_surface_emit", ctx, field, m, level, workspace, workspace_bytes)) return rc;
  if (verts_capacity < 0 || tris_capacity < 0 || (!verts && verts_capacity > 0) || (!faces && tris_capacity > 0) ||
      !isfinite(half_extent) || !(half_extent > 0.f)) {
    set_error("holo_surface_emit: capacities >= 0 with their buffers, half_extent > 0");
    return HOLO_E_INVALID;
  }
  return surface_emit_launch(field, m, level, half_extent, verts, verts_capacity, faces, tris_capacity, workspace, stream);
}

}  // extern "C"
