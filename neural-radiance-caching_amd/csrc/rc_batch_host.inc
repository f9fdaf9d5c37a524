// ---------------------------------------------------------------------------------------------------------
// rc_cast_rays / rc_cast_rays_multi / rc_train_batch: rays of one camera (rc_camera.hip), of mixed cameras and the
// training batch of one step (rc_batch.hip)
// ---------------------------------------------------------------------------------------------------------
// Argument errors of rc_cast_rays_multi and rc_train_batch are reported before the handle is looked at, into the handle's message or, without
// one, into the message rc_last_error(NULL) returns: a host can check a call's shape on a machine without a GPU.
static int batch_fail(rc_handle* h, const std::string& msg) {
  if (h) return fail(h, RC_ERR_INVALID_ARG, msg);
  g_create_error = msg;
  return RC_ERR_INVALID_ARG;
}

static RcCastOut cast_out(const rc_cast_outputs* out) {
  RcCastOut o{};
  o.origins = out->origins; o.directions = out->directions; o.viewdirs = out->viewdirs; o.radii = out->radii;
  o.imageplane = out->imageplane; o.look = out->look; o.up = out->up; o.lights = out->lights; o.near = out->near; o.far = out->far;
  return o;
}

// The fields rc_camera and rc_camera_set share, into the kernels' form; -> what is wrong with them, or NULL
template <class Cam>
static const char* cast_shared(const Cam* cam, RcCastShared& s) {
  if (cam->camtype < 0 || cam->camtype > 3)
    return "camtype must be 0 (perspective), 1 (panoramic), 2 (fisheye) or 3 (fisheye, equisolid)";
  s.near_v = cam->near; s.far_v = cam->far; s.camtype = cam->camtype;
  s.has_distortion = cam->has_distortion != 0;
  for (int i = 0; i < 6; ++i) s.dist[i] = cam->distortion[i];
  s.has_ndc = cam->has_ndc != 0;
  if (s.has_ndc) {          // convert_to_ndc: xmult = 1 / pixtocam[0, 2], ymult = 1 / pixtocam[1, 2] (camera_utils.py:97-98)
    if (cam->pixtocam_ndc[2] == 0.0f || cam->pixtocam_ndc[5] == 0.0f) return "pixtocam_ndc[0][2] and [1][2] must be non-zero";
    s.ndc_xmult = 1.0f / cam->pixtocam_ndc[2]; s.ndc_ymult = 1.0f / cam->pixtocam_ndc[5];
  }
  s.has_z_range = cam->has_z_range != 0; s.z_lo = cam->z_range[0]; s.z_hi = cam->z_range[1];
  return nullptr;
}

static const char* camera_tables(const rc_camera_set* set, RcCameraTables& t, RcCastShared& s) {
  if (set->count < 1) return "rc_camera_set.count must be at least 1";
  if (!set->pixtocams || !set->camtoworlds) return "rc_camera_set.pixtocams / camtoworlds are NULL";
  t.count = set->count; t.pixtocams = set->pixtocams; t.camtoworlds = set->camtoworlds; t.lights = set->lights;
  return cast_shared(set, s);
}

int rc_cast_rays_multi(rc_handle* h, const rc_camera_set* set, const int32_t* cam_idx, const int32_t* pix_x,
                       const int32_t* pix_y, int64_t n, const float* pix_dx, const float* pix_dy,
                       const rc_cast_outputs* out, void* stream_v) {
  RC_TRY
  if (!set || !out) return batch_fail(h, "rc_cast_rays_multi: null camera set/outputs");
  if (n < 0) return batch_fail(h, "rc_cast_rays_multi: negative n");
  RcCastMultiArgs a{};
  if (const char* bad = camera_tables(set, a.cams, a.s)) return batch_fail(h, std::string("rc_cast_rays_multi: ") + bad);
  if (n > 0 && (!cam_idx || !pix_x || !pix_y)) return batch_fail(h, "rc_cast_rays_multi: cam_idx, pix_x and pix_y are required");
  if ((pix_dx == nullptr) != (pix_dy == nullptr)) return batch_fail(h, "rc_cast_rays_multi: pix_dx and pix_dy go together");
  if (!h) return batch_fail(h, "rc_cast_rays_multi: null handle");
  if (n == 0) return RC_OK;
  RC_HIP(h, hipSetDevice(h->device));
  a.n = n; a.cam_idx = cam_idx; a.pix_x = pix_x; a.pix_y = pix_y; a.pix_dx = pix_dx; a.pix_dy = pix_dy;
  a.out = cast_out(out);
  rc_launch_cast_rays_multi(a, (hipStream_t)stream_v);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

int rc_train_batch(rc_handle* h, const rc_camera_set* set, const void* images, int32_t image_dtype, int32_t height,
                   int32_t width, const float* cam_lossmult, const uint32_t key[2], int32_t patch_size, int32_t border,
                   int32_t batching, int64_t n, const rc_train_batch_outputs* out, void* stream_v) {
  RC_TRY
  if (!set || !out) return batch_fail(h, "rc_train_batch: null camera set/outputs");
  if (!key) return batch_fail(h, "rc_train_batch: null key");
  if (n < 0) return batch_fail(h, "rc_train_batch: negative n");
  RcTrainBatchArgs a{};
  if (const char* bad = camera_tables(set, a.cams, a.s)) return batch_fail(h, std::string("rc_train_batch: ") + bad);
  if (!images) return batch_fail(h, "rc_train_batch: images is NULL");
  if (image_dtype != RC_IMAGE_F32 && image_dtype != RC_IMAGE_U8) return batch_fail(h, "rc_train_batch: image_dtype must be RC_IMAGE_F32 or RC_IMAGE_U8");
  if (batching != RC_BATCHING_ALL_IMAGES && batching != RC_BATCHING_SINGLE_IMAGE) return batch_fail(h, "rc_train_batch: unknown batching");
  if (height < 1 || width < 1 || patch_size < 1 || border < 0) return batch_fail(h, "rc_train_batch: height, width, patch_size must be positive and border non-negative");
  // datasets.py:966-971: x in [border, W - border - p + 1), y in [border, H - border - p + 1)
  const int64_t x_range = (int64_t)width - 2 * (int64_t)border - patch_size + 1;
  const int64_t y_range = (int64_t)height - 2 * (int64_t)border - patch_size + 1;
  if (x_range < 1 || y_range < 1) return batch_fail(h, "rc_train_batch: no admissible patch position (W - 2 border - p + 1 and H - 2 border - p + 1 must be at least 1)");
  const int64_t pp = (int64_t)patch_size * patch_size;
  if (n % pp != 0) return batch_fail(h, "rc_train_batch: n must be P * patch_size^2");
  const int64_t words = 3 * (n / pp);
  if (words >= 0xFFFFFFFFll) return batch_fail(h, "rc_train_batch: 3 P must be below 2^32 - 1");
  if ((set->pix_dx == nullptr) != (set->pix_dy == nullptr)) return batch_fail(h, "rc_train_batch: pix_dx and pix_dy go together");
  if (!h) return batch_fail(h, "rc_train_batch: null handle");
  if (n == 0) return RC_OK;
  RC_HIP(h, hipSetDevice(h->device));
  a.n = n; a.images = images; a.image_u8 = image_dtype == RC_IMAGE_U8; a.height = height; a.width = width;
  a.cam_lossmult = cam_lossmult; a.key0 = key[0]; a.key1 = key[1]; a.n_words = (uint32_t)words;
  a.patch = patch_size; a.x_lo = border; a.x_range = (int32_t)x_range; a.y_lo = border; a.y_range = (int32_t)y_range;
  a.single_image = batching == RC_BATCHING_SINGLE_IMAGE;
  a.pix_dx = set->pix_dx; a.pix_dy = set->pix_dy;
  a.out = cast_out(&out->rays);
  a.rgb = out->rgb; a.lossmult = out->lossmult; a.cam_idx = out->cam_idx; a.pix_x = out->pix_x; a.pix_y = out->pix_y;
  rc_launch_train_batch(a, (hipStream_t)stream_v);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

int rc_cast_rays(rc_handle* h, const rc_camera* cam, const int32_t* pix_x, const int32_t* pix_y, int64_t n,
                 int32_t x0, int32_t y0, int32_t width, int32_t height, const rc_cast_outputs* out, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (!cam || !out) return fail(h, RC_ERR_INVALID_ARG, "rc_cast_rays: null camera/outputs");
  if ((pix_x == nullptr) != (pix_y == nullptr)) return fail(h, RC_ERR_INVALID_ARG, "rc_cast_rays: pix_x and pix_y go together");
  if (!pix_x) {
    if (width <= 0 || height <= 0) return fail(h, RC_ERR_INVALID_ARG, "rc_cast_rays: empty pixel rectangle");
    if (n != (int64_t)width * height) return fail(h, RC_ERR_INVALID_ARG, "rc_cast_rays: n must equal width * height");
  }
  if (n < 0) return fail(h, RC_ERR_INVALID_ARG, "rc_cast_rays: negative n");
  if (n == 0) return RC_OK;
  RC_HIP(h, hipSetDevice(h->device));
  RcCastArgs a{};
  a.n = n; a.pix_x = pix_x; a.pix_y = pix_y; a.x0 = x0; a.y0 = y0; a.width = width > 0 ? width : 1;
  for (int i = 0; i < 9; ++i) a.pixtocam[i] = cam->pixtocam[i];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) a.rot[3 * r + c] = cam->camtoworld[4 * r + c];
    a.trans[r] = cam->camtoworld[4 * r + 3];
    a.light[r] = cam->light[r];
  }
  if (const char* bad = cast_shared(cam, a.s))
    return fail(h, cam->camtype < 0 || cam->camtype > 3 ? RC_ERR_UNSUPPORTED : RC_ERR_INVALID_ARG, std::string("rc_cast_rays: ") + bad);
  if ((cam->pix_dx == nullptr) != (cam->pix_dy == nullptr)) return fail(h, RC_ERR_INVALID_ARG, "rc_cast_rays: pix_dx and pix_dy go together");
  a.pix_dx = cam->pix_dx; a.pix_dy = cam->pix_dy;
  a.out = cast_out(out);
  rc_launch_cast_rays(a, (hipStream_t)stream_v);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}
