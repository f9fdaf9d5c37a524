// On-device ray generation for pinhole and panoramic cameras.
//
// Replaces camera_utils.pixels_to_rays (internal/camera_utils.py:896-1072) + cast_ray_batch (:1225-1329), one camera per
// call: ProjectionType.PERSPECTIVE (the BASELINE scenes), PANORAMIC (= cast_spherical_rays, :1415-1443, the secondary-ray
// visualisation), FISHEYE / FISHEYE_EQUISOLID (:991-1011), radial + tangential distortion undone by the reference's 10
// Newton steps (:795-890), NDC rays (convert_to_ndc, :50-111, radii from the NDC origin offsets :1058-1066), sub-pixel
// jitter offsets handed over as tensors (:943-957), z_range cropping (:1143-1164, 1291-1299).  Same arithmetic in the
// same order: pixel centre (x + 0.5, y + 0.5, 1) and its +1 neighbours in x and y through pixtocam, flip to OpenGL axes (y, z negated), rotate by camtoworld[:3, :3],
// viewdirs = directions / |directions|, radii = 0.5 (|dx - d| + |dy - d|) * 2 / sqrt(12).
#include "rc_internal.h"
#include "rc_dev_camera.h"

namespace {

__global__ void k_cast_rays(RcCastArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  int px, py;
  if (a.pix_x) {
    px = a.pix_x[i]; py = a.pix_y[i];
  } else {
    px = a.x0 + (int)(i % a.width); py = a.y0 + (int)(i / a.width);
  }
  const bool jit = a.pix_dx != nullptr;
  const RcCastRow row = cast_pixel(a.s, a.pixtocam, a.rot, a.trans, px, py, jit, jit ? a.pix_dx[i] : 0.0f, jit ? a.pix_dy[i] : 0.0f);
  store_cast_row(a.out, i, row, a.rot, a.light, a.s.near_v, a.s.far_v);
}

}  // namespace

void rc_launch_cast_rays(const RcCastArgs& a, hipStream_t stream) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_cast_rays, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, stream, a);
}
