// Host side of rc_probe_rays and rc_vmf_panorama (rc_probe.hip, DESIGN.md §4.21); included by rc_api.hip.
//
// Both calls check every argument before anything is launched, keep no state on the handle and allocate nothing: one
// launch each, ordered on the stream.

// What is wrong with the panorama of P probes, or NULL
static const char* probe_panorama_fault(int32_t P, int32_t height, int32_t width) {
  if (P < 1 || P > RC_PROBE_MAX) return "P must be in [1, 16]";
  if (height < 1 || width < 1) return "height and width must be at least 1";
  if ((int64_t)P * height * width >= (1ll << 31)) return "P height width must be below 2^31";
  return nullptr;
}

// The half-pixel offsets of utils.get_sphere_directions: Python doubles, rounded once where they meet the float32 grid
static void probe_offsets(int32_t height, int32_t width, float& phi_offset, float& theta_offset) {
  const double pi = 3.14159265358979323846;
  phi_offset = (float)(2.0 * pi / (2.0 * width));
  theta_offset = (float)(pi / (2.0 * height));
}

int rc_probe_rays(rc_handle* h, const rc_probe_view* view, const int64_t* pixel, int32_t P, int32_t height, int32_t width,
                  float near_v, float far_v, float normal_offset, int32_t flip, const rc_cast_outputs* out, float* positions,
                  void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_probe_rays";
  if (!view || !pixel || !out) return fail(h, RC_ERR_INVALID_ARG, who + ": null view/pixel/outputs");
  if (!view->origins || !view->directions || !view->distance_median || !view->normals)
    return fail(h, RC_ERR_INVALID_ARG, who + ": origins, directions, distance_median and normals are required");
  if (const char* bad = probe_panorama_fault(P, height, width)) return fail(h, RC_ERR_INVALID_ARG, who + ": " + bad);
  for (int p = 0; p < P; ++p)
    if (pixel[p] < 0 || pixel[p] >= view->n_view)
      return fail(h, RC_ERR_INVALID_ARG, who + ": pixel[" + std::to_string(p) + "] = " + std::to_string(pixel[p]) +
                                             " is outside the view's " + std::to_string(view->n_view) + " rows");
  RcProbeRaysArgs a{};
  a.out = cast_out(out);
  a.positions = positions;
  const RcCastOut& o = a.out;
  if (!positions && !o.origins && !o.directions && !o.viewdirs && !o.radii && !o.imageplane && !o.look && !o.up && !o.lights &&
      !o.near && !o.far)
    return fail(h, RC_ERR_INVALID_ARG, who + ": no output requested");
  RoctxScope roctx_call("rc_probe_rays");
  RC_HIP(h, hipSetDevice(h->device));
  a.origins = view->origins; a.directions = view->directions; a.distance_median = view->distance_median;
  a.normals = view->normals; a.lights = view->lights; a.imageplane = view->imageplane; a.look = view->look; a.up = view->up;
  for (int p = 0; p < P; ++p) a.pixel[p] = pixel[p];
  a.P = P; a.height = height; a.width = width; a.flip = flip != 0;
  a.n = (int64_t)P * height * width;
  a.normal_offset = normal_offset;
  probe_offsets(height, width, a.phi_offset, a.theta_offset);
  // cast_spherical_rays (camera_utils.py:1415-1443): pixtocam = diag(2 pi / W, pi / H, 1) in double, rounded as the
  // binding rounds a camera's; the rotation is the identity the reference ends up with (trainer.py:880)
  const double pi = 3.14159265358979323846;
  a.pixtocam[0] = (float)(2.0 * pi / width); a.pixtocam[4] = (float)(pi / height); a.pixtocam[8] = 1.0f;
  a.rot[0] = a.rot[4] = a.rot[8] = 1.0f;
  a.s.near_v = near_v; a.s.far_v = far_v; a.s.camtype = 1;
  rc_launch_probe_rays(a, (hipStream_t)stream_v);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

int rc_vmf_panorama(rc_handle* h, const float* means, const float* kappas, const float* logits, int32_t P, int32_t V,
                    int32_t height, int32_t width, int32_t flip, float* out_linear, float* out_srgb, uint8_t* out_u8,
                    void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_vmf_panorama";
  if (!means || !kappas || !logits) return fail(h, RC_ERR_INVALID_ARG, who + ": means, kappas and logits are required");
  if (const char* bad = probe_panorama_fault(P, height, width)) return fail(h, RC_ERR_INVALID_ARG, who + ": " + bad);
  if (V < 1 || V > RC_PROBE_MAX_LOBES) return fail(h, RC_ERR_INVALID_ARG, who + ": V must be in [1, 128]");
  if (!out_linear && !out_srgb && !out_u8) return fail(h, RC_ERR_INVALID_ARG, who + ": no output requested");
  RoctxScope roctx_call("rc_vmf_panorama");
  RC_HIP(h, hipSetDevice(h->device));
  RcVmfPanoramaArgs a{};
  a.means = means; a.kappas = kappas; a.logits = logits;
  a.V = V; a.height = height; a.width = width; a.flip = flip != 0;
  probe_offsets(height, width, a.phi_offset, a.theta_offset);
  a.out_linear = out_linear; a.out_srgb = out_srgb; a.out_u8 = out_u8;
  rc_launch_vmf_panorama(a, P, (hipStream_t)stream_v);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}
