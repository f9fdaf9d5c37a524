// The workspace registry of the host layer: every buffer set, its rc_workspace_ptr prefix and the names of its buffers,
// declared once.  No HIP type in here: rc_api.hip adds the stream and event bookkeeping of a set (WsSet) on top of WsBufs,
// hostcheck.cpp walks the registry on the CPU under the sanitizers.
//
// Adding a set: write its struct of WsBuf, give it an entry in RC_WS_SETS, list its buffers in
// wsn::kTable.  The static_assert behind the table refuses a struct with an unlisted buffer.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <type_traits>
#include <utility>
#include <variant>

#include "../../include/rc_abi.h"

// Workspace buffer: device pointer, capacity in bytes, element count of the last request (rc_workspace_ptr).
struct WsBuf { float* p = nullptr; size_t bytes = 0; int64_t count = 0; };
// One set of rc_render_rays' launch-per-stage buffers (ensure_workspace).
struct RenderWs {
  WsBuf sdist[RC_MAX_LEVELS], tdist[RC_MAX_LEVELS], means[RC_MAX_LEVELS], feat[RC_MAX_LEVELS], density[RC_MAX_LEVELS],
      weights[RC_MAX_LEVELS];
  WsBuf hbuf, normals_pred, normals_grad, jac, app, shade, debug, env_rgb, rgb_noenv, acc_ws, inds, src_idx, filt_weight, acc_sel;
  WsBuf feat_sel, hbuf_sel, normals_sel, density_sel;   // lean resampling pass: the picked samples only
  WsBuf t_irr, t_slf, tshade;                          // time-resolved cache: set 0 only
};
// Set 0 only: rc_render_material's buffers and the shadow rays of rc_render_transient.
struct ExtraWs {
  WsBuf m_pts, m_nrm, m_feat, m_mat, m_feat_all, m_mat_all, l_feat, l_vmf, l_vmf_logit, sec_origins, sec_dirs, sec_near,
      sec_far, sec_lights, sec_samples, m_local_view, sec_rgb, sec_acc, sec_env;
  WsBuf sh_origins, sh_dirs, sh_near, sh_far, sh_normals, sh_lights, sh_acc;
};
// rc_density_backward.
struct TrainWs { WsBuf feat, dfeat, a1, a2, d1, d2, fe, graw, density, partial; };
// rc_interlevel_backward, beside its RenderWs (the training forward): per proposal level d loss / d density and the
// sample means as points [n S][3]; the per-ray loss sums.
struct InterlevelWs { WsBuf d_density[RC_MAX_LEVELS], points[RC_MAX_LEVELS]; WsBuf loss_ray; };
// rc_data_backward, beside its RenderWs (the training forward): the ray rgb, per-ray loss sums, per-sample d loss / d
// density and d loss / d rgb_s, the means as points [n S][3]; then one sample chunk of the shader backward
// (rc_data_host.inc; rc_train_host.inc's dense-layer helpers: recompute activations, their gradients, the weight-gradient
// K-slices and a column of ones).
struct DataWs {
  WsBuf rgb, loss_ray, d_density, d_rgbs, points;
  WsBuf f96, heads, p3, ib_in, x328, s0, s1, sb, i1, i2, io, so;
  WsBuf dheads, dio, dso, dsb, dx328, ds1, ds0, di2, di1, dib_in, db128, dp3, df96, dfeat, dapp, part, ones;
};
// rc_geometry_backward, beside its RenderWs (the training forward): per-ray values of the four terms, per-sample d loss /
// d density and d loss / d pred_raw, the means as points [n S][3]; one sample chunk of the hidden vectors h64 and
// d feature64, the weight-gradient K-slices and a column of ones; rc_density_regularizer's per-table partial sums.
struct GeometryWs { WsBuf loss_ray, d_density, d_pred, points, h64, dfeat, part, ones, reg_part; };
// rc_adam_update: the per-tile sums of g^2 (doubles), the norm and the clip multiplier; rc_load_params_flat: the dense
// segments of a layout gathered for the one copy to the host.
struct OptimWs { WsBuf part, norm, mult, stage; };
// rc_light_sampling_backward (its forward on set 0 and WS_SECONDARY): the primary pass's composite (not read), the light
// head's recompute and its gradients, the per-point loss sums, the weight-gradient K slices and a column of ones;
// rc_light_regularizer's per-table partial sums.
struct LightWs { WsBuf cache_rgb, cache_acc, h0, h1, vp, dvp, dh1, dh0, dfeat, loss_ray, part, ones, reg_part; };
// rc_material_smoothness_backward (its forward on set 0): the primary pass's composite (not read), the lookup points and
// features of both evaluations, the materials at x', the per-point and per-workgroup loss sums, d loss / d features, the
// per-workgroup weight-gradient partials; rc_material_regularizer's per-table partial sums.
struct MaterialWs { WsBuf cache_rgb, cache_acc, pts, feat, mat_p, loss_ray, loss_part, dfeat, part, reg_part; };
// rc_material_data_backward (its forward is rc_render_material on set 0 and WS_SECONDARY): the primary pass's composite
// ("cache_rgb" is read by the loss), the rebuilt rgb, the per-point loss sums and d loss / d material, d loss / d features,
// the per-workgroup weight-gradient partials and loss sums.
// rc_material_data_backward_env adds d loss / d (EnvMap radiance) per secondary ray and one row chunk of the EnvMap's
// backward (rc_envmap_bwd.hip): the recompute's activations (xb = [layer_2's output | the encoded direction]), their
// gradients, the weight-gradient K slices and a 1.0f.
struct MatDataWs {
  WsBuf cache_rgb, cache_acc, rgb, loss_ray, dmat, dfeat, part, loss_part;
  WsBuf d_env, e_h0, e_h1, e_xb, e_hb, e_raw, e_draw, e_dhb, e_dxb, e_dh1, e_dh0, e_part, e_ones;
};
// rc_transient_data_backward (its forward is rc_render_transient on set 0): the rendered histograms, G = d loss / d rgb and
// the temporal filter's transpose of it, the per-ray loss and mse sums; one chunk of kRcTdChunkRays rays of the heads'
// backward (dZ of both heads, their inputs row-major, the weight-gradient K slices, a 1.0f); the adjoints of everything
// k_transient_shader hands to k_transient_bins, for all n rays.
struct TransDataWs {
  WsBuf rgb, G, Gt, loss_ray, dz_irr, dz_slf, x_irr, x_slf, part, ones;
  WsBuf d_t_irr, d_t_slf, d_tint_ibrdf, d_direct, d_weights;
  WsBuf d_density, points;      // rc_transient_data_backward_sampler: d loss / d density through the weights, the means [n S][3]
};
// rc_eval_image: the bin sums of both histograms (n_bins > 0), the post-processed images where the caller gives no buffer
// of its own, and the per-workgroup partial sums of the three kernels (doubles).  rc_eval_shift_invariant: the metric maps
// of one di row of shifts, the search state ([4][H][W]: best pooled, best metric, di, dj) and the per-workgroup partial
// sums of both searches (doubles).
struct EvalWs { WsBuf binsum_pred, binsum_gt, post_pred, post_gt, part, si_metric, si_state, si_part; };
// rc_eval_albedo / rc_albedo_ratio: the view's own pair rows (no ratio handed in), the valid pixels per workgroup (int32),
// the select's state (RcAlbedoState) and the per-workgroup partial sums (doubles).
struct AlbedoWs { WsBuf pairs, wg, state, part; };
// rc_weighted_percentile / rc_image_max / rc_vis_images: the select's state (RcVisState), its per-workgroup weight sums
// (doubles), the per-workgroup maxima and the sums over the bins of the histogram images ([slots][H W][3]).
struct VisWs { WsBuf state, part, maxpart, binsum; };
// rc_mask_backward, beside its RenderWs (the training forward): the per-ray loss terms, per-sample d loss / d density and
// the means as points [n S][3].
struct MaskWs { WsBuf loss_ray, d_density, points; };
// rc_env_tables / rc_env_pick: the per-workgroup sums of the tables' normaliser (doubles) and the per-pick (score, texel)
// maxima (64-bit integers).
struct RelightWs { WsBuf part, best; };
// rc_normals_backward: the last level's grid features and their Jacobian, d raw / d feature (feature-major) and G^ = d L /
// d (the Jacobian-chained gradient) for the scatter, the point-major operands of the weight-gradient contraction
// (u [n][32]; t0, a0, t1, a2 [n][64]; a column of ones), its per-workgroup partials, and the normals when the caller wants none.
struct NormalsWs { WsBuf feat, jac, gf, ghat, u, t0, a0, t1, a2, ones, partial, normals; };
// rc_geometry_smoothness_backward, beside its RenderWs (the training forward): the perturbed means (SoA, as the density MLP
// reads them) with their features, Jacobian, density and analytic normals; the means and perturbed means as points [n S][3];
// d loss / d normals and d loss / d density at both point sets; the per-ray loss values.
struct GSmoothWs { WsBuf means_p, feat_p, jac_p, density_p, normals_p, points, points_p, d_normals, d_normals_p, d_density, d_density_p, loss_ray; };
// rc_query_points / rc_density_lattice, one chunk of points: the points as SoA [3][C], the grid features (feature-major)
// and their Jacobian, the density where the caller wants none, both kinds of normals as SoA, the material grid's features.
struct QueryWs { WsBuf means, feat, jac, density, normals_pred, normals_grad, m_feat; };
// rc_isosurface (RcIsoArgs): per lattice point the mask of crossing owned edges and the cell's triangle count (bytes) and
// the index of its first vertex (int32), per tile and per group the sums / offsets of both scans (int32; int64 pairs), the
// RcIsoState.
struct IsoWs { WsBuf mask, tcount, tile_v, tile_t, group_v, group_t, group_off, vbase, state; };
// rc_bake_atlas / rc_query_cache_diffuse, beside the QueryWs of WS_QUERY, one chunk: the texels' points as rows [C][3] and
// their owners (int32); the last level's hidden vectors (k_density_mlp's accumulator layout) and the appearance grid's
// features (feature-major).
struct AtlasWs { WsBuf points, owner, hidden, app_feat; };

// Workspace sets: X(id, rc_workspace_ptr's "<prefix><name>", the extra struct its entry points put into it), B(id, prefix)
// for a set that holds a RenderWs and nothing else.  The enum, the prefixes and the variant of the extra structs all come
// from this list.
// WS_RENDER0-3 serve rc_render_rays, one per caller stream, so that independent batches enqueued on different streams
// overlap (the least recently used one is taken over when a fifth stream shows up); WS_RENDER0 also serves
// rc_render_material / rc_render_transient (with ExtraWs), whose batched secondary trace runs on WS_SECONDARY.
// WS_LIGHT, WS_MATERIAL and WS_MATDATA hold the buffers of the material-stage losses' own (their forward runs on WS_RENDER0
// + WS_SECONDARY), WS_TRANSDATA those of rc_transient_data_backward (its forward is rc_render_transient's, on WS_RENDER0),
// WS_ATLAS those of rc_bake_atlas and rc_query_cache_diffuse's own (their query launches run on WS_QUERY); WS_GEOMETRY,
// WS_LIGHT and WS_MATERIAL also serve their stage's regularizer.  Every other set serves the entry points named at its struct.
#define RC_WS_SETS(X, B)                                                                                                \
  X(RENDER0, "", ExtraWs) B(RENDER1, "p1:") B(RENDER2, "p2:") B(RENDER3, "p3:") B(SECONDARY, "s:") X(TRAIN, "t:", TrainWs)  \
  X(INTERLEVEL, "i:", InterlevelWs) X(DATA, "d:", DataWs) X(GEOMETRY, "g:", GeometryWs) X(OPTIM, "o:", OptimWs)         \
  X(LIGHT, "ls:", LightWs) X(MATERIAL, "ms:", MaterialWs) X(MATDATA, "md:", MatDataWs) X(TRANSDATA, "td:", TransDataWs) \
  X(EVAL, "ev:", EvalWs) X(ALBEDO, "ea:", AlbedoWs) X(VIS, "vz:", VisWs) X(MASK, "mk:", MaskWs)                         \
  X(RELIGHT, "rl:", RelightWs) X(NORMALS, "nb:", NormalsWs) X(GSMOOTH, "gs:", GSmoothWs) X(QUERY, "q:", QueryWs)        \
  X(ISO, "iso:", IsoWs) X(ATLAS, "atlas:", AtlasWs)

#define RC_WS_ID(id, ...) WS_##id,
enum WsSetId { RC_WS_SETS(RC_WS_ID, RC_WS_ID) WS_COUNT };
#undef RC_WS_ID

// The extra buffers a set holds beside its RenderWs: of the kind its entry point uses, fixed by that entry point's first call.
#define RC_WS_STRUCT(id, prefix, X) , X
#define RC_WS_NONE(id, prefix)
using WsExtra = std::variant<std::monostate RC_WS_SETS(RC_WS_STRUCT, RC_WS_NONE)>;
#undef RC_WS_STRUCT
#undef RC_WS_NONE
struct WsBufs {
  RenderWs r;
  WsExtra x;
};

namespace wsn {
// index of alternative X in WsExtra; the std::monostate slot, 0, stands for RenderWs in WsName::kind
template <class X, size_t I = 0> constexpr size_t kind_of() {
  if constexpr (std::is_same_v<X, RenderWs>) return 0;
  else if constexpr (std::is_same_v<X, std::variant_alternative_t<I, WsExtra>>) return I;
  else return kind_of<X, I + 1>();
}
template <class X> X* held(WsBufs& s) {
  if constexpr (std::is_same_v<X, RenderWs>) return &s.r;
  else return std::get_if<X>(&s.x);
}
}  // namespace wsn

struct WsSetInfo { const char* prefix; size_t kind; };
#define RC_WS_INFO(id, prefix, X) {prefix, wsn::kind_of<X>()},
#define RC_WS_BARE(id, prefix) {prefix, 0},
constexpr WsSetInfo kWsSets[WS_COUNT] = {RC_WS_SETS(RC_WS_INFO, RC_WS_BARE)};
#undef RC_WS_INFO
#undef RC_WS_BARE

// One named buffer (per-level buffers: RC_MAX_LEVELS of them, "<name><level>") of the struct of kind `kind`.
struct WsName {
  const char* name;
  size_t kind;
  int count;                             // 1, or RC_MAX_LEVELS of a per-level buffer
  int fewer;                             // per-level buffers: how many levels short of num_levels the digits stop
  WsBuf* (*at)(WsBufs&, int);            // the buffer in a set (level l of a per-level buffer); nullptr when the set holds another kind
};
namespace wsn {
template <auto M> struct Member;
template <class X, WsBuf X::*M> struct Member<M> {
  static constexpr size_t kind = kind_of<X>();
  static constexpr int count = 1;
  static WsBuf* at(WsBufs& s, int) { X* p = held<X>(s); return p ? &(p->*M) : nullptr; }
};
template <class X, WsBuf (X::*M)[RC_MAX_LEVELS]> struct Member<M> {
  static constexpr size_t kind = kind_of<X>();
  static constexpr int count = RC_MAX_LEVELS;
  static WsBuf* at(WsBufs& s, int l) { X* p = held<X>(s); return p ? &(p->*M)[l] : nullptr; }
};
template <auto M> constexpr WsName row(const char* name, int fewer = 0) { return {name, Member<M>::kind, Member<M>::count, fewer, &Member<M>::at}; }

#define WS(S, m) row<&S::m>(#m)
constexpr WsName kTable[] = {
    WS(RenderWs, sdist), WS(RenderWs, tdist), WS(RenderWs, means), WS(RenderWs, feat), WS(RenderWs, density), WS(RenderWs,
    weights), WS(RenderWs, hbuf), WS(RenderWs, normals_pred), WS(RenderWs, normals_grad), WS(RenderWs, jac), WS(RenderWs, app),
    WS(RenderWs, shade), WS(RenderWs, debug), WS(RenderWs, env_rgb), WS(RenderWs, rgb_noenv), WS(RenderWs, acc_ws), WS(RenderWs,
    inds), WS(RenderWs, src_idx), WS(RenderWs, filt_weight), WS(RenderWs, acc_sel), WS(RenderWs, feat_sel), WS(RenderWs,
    hbuf_sel), WS(RenderWs, normals_sel), WS(RenderWs, density_sel), WS(RenderWs, t_irr), WS(RenderWs, t_slf), WS(RenderWs,
    tshade), WS(ExtraWs, m_pts), WS(ExtraWs, m_nrm), WS(ExtraWs, m_feat), WS(ExtraWs, m_mat), WS(ExtraWs, m_feat_all),
    WS(ExtraWs, m_mat_all), WS(ExtraWs, l_feat), WS(ExtraWs, l_vmf), WS(ExtraWs, l_vmf_logit), WS(ExtraWs, sec_origins),
    WS(ExtraWs, sec_dirs), WS(ExtraWs, sec_near), WS(ExtraWs, sec_far), WS(ExtraWs, sec_lights), WS(ExtraWs, sec_samples),
    WS(ExtraWs, m_local_view), WS(ExtraWs, sec_rgb), WS(ExtraWs, sec_acc), WS(ExtraWs, sec_env), WS(ExtraWs, sh_origins),
    WS(ExtraWs, sh_dirs), WS(ExtraWs, sh_near), WS(ExtraWs, sh_far), WS(ExtraWs, sh_normals), WS(ExtraWs, sh_lights),
    WS(ExtraWs, sh_acc), WS(TrainWs, feat), WS(TrainWs, dfeat), WS(TrainWs, a1), WS(TrainWs, a2), WS(TrainWs, d1), WS(TrainWs,
    d2), WS(TrainWs, fe), WS(TrainWs, graw), WS(TrainWs, density), WS(TrainWs, partial),
    // the interlevel loss has no gradient for the last level: its per-level buffers stop one level short
    row<&InterlevelWs::d_density>("d_density", 1), row<&InterlevelWs::points>("points", 1), WS(InterlevelWs, loss_ray),
    WS(DataWs, rgb), WS(DataWs, loss_ray), WS(DataWs, d_density), WS(DataWs, d_rgbs), WS(DataWs, points), WS(DataWs, f96),
    WS(DataWs, heads), WS(DataWs, p3), WS(DataWs, ib_in), WS(DataWs, x328), WS(DataWs, s0), WS(DataWs, s1), WS(DataWs, sb),
    WS(DataWs, i1), WS(DataWs, i2), WS(DataWs, io), WS(DataWs, so), WS(DataWs, dheads), WS(DataWs, dio), WS(DataWs, dso),
    WS(DataWs, dsb), WS(DataWs, dx328), WS(DataWs, ds1), WS(DataWs, ds0), WS(DataWs, di2), WS(DataWs, di1), WS(DataWs, dib_in),
    WS(DataWs, db128), WS(DataWs, dp3), WS(DataWs, df96), WS(DataWs, dfeat), WS(DataWs, dapp), WS(DataWs, part), WS(DataWs,
    ones), WS(GeometryWs, loss_ray), WS(GeometryWs, d_density), WS(GeometryWs, d_pred), WS(GeometryWs, points), WS(GeometryWs,
    h64), WS(GeometryWs, dfeat), WS(GeometryWs, part), WS(GeometryWs, ones), WS(GeometryWs, reg_part), WS(OptimWs, part),
    WS(OptimWs, norm), WS(OptimWs, mult), WS(OptimWs, stage), WS(LightWs, cache_rgb), WS(LightWs, cache_acc), WS(LightWs, h0),
    WS(LightWs, h1), WS(LightWs, vp), WS(LightWs, dvp), WS(LightWs, dh1), WS(LightWs, dh0), WS(LightWs, dfeat), WS(LightWs,
    loss_ray), WS(LightWs, part), WS(LightWs, ones), WS(LightWs, reg_part), WS(MaterialWs, cache_rgb), WS(MaterialWs,
    cache_acc), WS(MaterialWs, pts), WS(MaterialWs, feat), WS(MaterialWs, mat_p), WS(MaterialWs, loss_ray), WS(MaterialWs,
    loss_part), WS(MaterialWs, dfeat), WS(MaterialWs, part), WS(MaterialWs, reg_part), WS(MatDataWs, cache_rgb), WS(MatDataWs,
    cache_acc), WS(MatDataWs, rgb), WS(MatDataWs, loss_ray), WS(MatDataWs, dmat), WS(MatDataWs, dfeat), WS(MatDataWs, part),
    WS(MatDataWs, loss_part), WS(MatDataWs, d_env), WS(MatDataWs, e_h0), WS(MatDataWs, e_h1), WS(MatDataWs, e_xb), WS(MatDataWs,
    e_hb), WS(MatDataWs, e_raw), WS(MatDataWs, e_draw), WS(MatDataWs, e_dhb), WS(MatDataWs, e_dxb), WS(MatDataWs, e_dh1),
    WS(MatDataWs, e_dh0), WS(MatDataWs, e_part), WS(MatDataWs, e_ones), WS(TransDataWs, rgb), WS(TransDataWs, G),
    WS(TransDataWs, Gt), WS(TransDataWs, loss_ray), WS(TransDataWs, dz_irr), WS(TransDataWs, dz_slf), WS(TransDataWs, x_irr),
    WS(TransDataWs, x_slf), WS(TransDataWs, part), WS(TransDataWs, ones), WS(TransDataWs, d_t_irr), WS(TransDataWs, d_t_slf),
    WS(TransDataWs, d_tint_ibrdf), WS(TransDataWs, d_direct), WS(TransDataWs, d_weights), WS(TransDataWs, d_density),
    WS(TransDataWs, points), WS(EvalWs, binsum_pred), WS(EvalWs, binsum_gt), WS(EvalWs, post_pred), WS(EvalWs, post_gt),
    WS(EvalWs, part), WS(EvalWs, si_metric), WS(EvalWs, si_state), WS(EvalWs, si_part), WS(AlbedoWs, pairs), WS(AlbedoWs, wg),
    WS(AlbedoWs, state), WS(AlbedoWs, part), WS(VisWs, state), WS(VisWs, part), WS(VisWs, maxpart), WS(VisWs, binsum),
    WS(MaskWs, loss_ray), WS(MaskWs, d_density), WS(MaskWs, points), WS(RelightWs, part), WS(RelightWs, best), WS(NormalsWs,
    feat), WS(NormalsWs, jac), WS(NormalsWs, gf), WS(NormalsWs, ghat), WS(NormalsWs, u), WS(NormalsWs, t0), WS(NormalsWs, a0),
    WS(NormalsWs, t1), WS(NormalsWs, a2), WS(NormalsWs, ones), WS(NormalsWs, partial), WS(NormalsWs, normals), WS(GSmoothWs,
    means_p), WS(GSmoothWs, feat_p), WS(GSmoothWs, jac_p), WS(GSmoothWs, density_p), WS(GSmoothWs, normals_p), WS(GSmoothWs,
    points), WS(GSmoothWs, points_p), WS(GSmoothWs, d_normals), WS(GSmoothWs, d_normals_p), WS(GSmoothWs, d_density),
    WS(GSmoothWs, d_density_p), WS(GSmoothWs, loss_ray), WS(QueryWs, means), WS(QueryWs, feat), WS(QueryWs, jac), WS(QueryWs,
    density), WS(QueryWs, normals_pred), WS(QueryWs, normals_grad), WS(QueryWs, m_feat), WS(IsoWs, mask), WS(IsoWs, tcount),
    WS(IsoWs, tile_v), WS(IsoWs, tile_t), WS(IsoWs, group_v), WS(IsoWs, group_t), WS(IsoWs, group_off), WS(IsoWs, vbase),
    WS(IsoWs, state), WS(AtlasWs, points), WS(AtlasWs, owner), WS(AtlasWs, hidden), WS(AtlasWs, app_feat)};
#undef WS
// every struct, RenderWs (kind 0) included, is exactly the WsBufs the table lists for it
constexpr size_t listed(size_t kind) { size_t n = 0; for (const WsName& e : kTable) n += e.kind == kind ? e.count : 0; return n; }
template <size_t K> constexpr size_t bufs_of() { return (K ? sizeof(std::variant_alternative_t<K, WsExtra>) : sizeof(RenderWs)) / sizeof(WsBuf); }
template <size_t... K> constexpr bool complete(std::index_sequence<K...>) { return ((listed(K) == bufs_of<K>()) && ...); }
static_assert(complete(std::make_index_sequence<std::variant_size_v<WsExtra>>()), "the table lists every workspace buffer of every struct");
}  // namespace wsn

// f(buffer) on every buffer the set holds (rc_destroy frees them).
template <class F> void ws_for_each(WsBufs& s, F f) {
  for (const WsName& e : wsn::kTable)
    for (int l = 0; l < e.count; ++l)
      if (WsBuf* b = e.at(s, l)) f(*b);
}

// rc_workspace_ptr: "<set prefix><name>[level]" -> the set's id and the name behind the prefix (-1 for an unknown prefix)
inline int ws_split(const char* name, std::string& leaf) {
  const char* colon = strchr(name, ':');
  const std::string pre = colon ? std::string(name, colon + 1) : "";
  leaf = colon ? colon + 1 : name;
  for (int set = 0; set < WS_COUNT; ++set)
    if (pre == kWsSets[set].prefix) return set;
  return -1;
}
// ... and the buffer `leaf` names in set `s` of a config with num_levels levels: a name resolves in RenderWs or in the
// struct the set holds, the table's first match winning (nullptr for an unknown name)
inline WsBuf* ws_lookup(WsBufs& s, const std::string& leaf, int num_levels) {
  for (const WsName& e : wsn::kTable) {
    const size_t k = strlen(e.name);
    if (leaf.compare(0, k, e.name) != 0) continue;
    WsBuf* b = nullptr;
    if (leaf.size() == k) b = e.count == 1 ? e.at(s, 0) : nullptr;
    else if (e.count > 1 && leaf.size() == k + 1 && leaf[k] >= '0' && leaf[k] < '0' + num_levels - e.fewer) b = e.at(s, leaf[k] - '0');
    if (b) return b;
  }
  return nullptr;
}
