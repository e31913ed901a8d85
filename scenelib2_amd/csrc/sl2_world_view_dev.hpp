// The world view and picking: the arithmetic of sl2_world_items and of sl2_pick_items_* -
// include/scenelib2_amd.h, "the world view and picking" - as SL2_HD functions.  The same source is the body of k_world_list and
// k_pick_items (sl2_world_view.hip) and of sl2_pick_items_host, and a stand-alone host program can include it
// (tests/world_view_host.cpp): the forms agree bit for bit by construction, given -ffp-contract=off and correctly rounded FP64
// division on both sides.  The projection, the conic and the 3-D segment rule are sl2_rectify_dev.hpp's, unchanged: the view
// takes the place of the sequence's camera.
#pragma once
#include "../../include/scenelib2_amd.h"
#include "sl2_math.hpp"
#include "sl2_overlay_dev.hpp"
#include "sl2_rectify_dev.hpp"

namespace sl2 {

constexpr int kWorldGlyphEdges = 16;      // DrawCamera as wire: 12 edges of the body box, 4 of the lens's front face
constexpr int kWorldAxes = 3;

// The view's pose as the seven numbers zeroedyi_only takes
SL2_HD void world_view_pose(const sl2_view& v, double xp[7]) {
  xp[0] = v.r[0]; xp[1] = v.r[1]; xp[2] = v.r[2];
  xp[3] = v.q[0]; xp[4] = v.q[1]; xp[5] = v.q[2]; xp[6] = v.q[3];
}

// m = RRW (y - r) and Jy = RRW of the view: zeroedyi_only's expressions, the rotation kept
SL2_HD void world_zeroed(const double xp[7], const double y[3], double m[3], double Jy[9]) {
  const double d[3] = {y[0] - xp[0], y[1] - xp[1], y[2] - xp[2]};
  double qi[4];
  quat_inverse(&xp[3], qi);
  quat_to_rot(qi, Jy);
  for (int i = 0; i < 3; ++i) {
    double acc = 0.0;
    for (int k = 0; k < 3; ++k) acc += Jy[i * 3 + k] * d[k];
    m[i] = acc;
  }
}

// Sigma = (Jy Pyy) Jy^T in the header's order: every inner sum starts at 0.0 and runs upwards
SL2_HD void world_sigma(const double Jy[9], const double Pyy[9], double Sg[9]) {
  double C[9];
  for (int i = 0; i < 3; ++i)
    for (int c = 0; c < 3; ++c) {
      double acc = 0.0;
      for (int k = 0; k < 3; ++k) acc += Jy[i * 3 + k] * Pyy[k * 3 + c];
      C[i * 3 + c] = acc;
    }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double acc = 0.0;
      for (int c = 0; c < 3; ++c) acc += C[i * 3 + c] * Jy[j * 3 + c];
      Sg[i * 3 + j] = acc;
    }
}

// The two ends of glyph edge e (0 .. 15) in the glyph's own frame: the header's edge order, computed from the bits of e (no
// table: an index known only at run time would put one in scratch)
SL2_HD void world_glyph_edge(int e, double a[3], double b[3]) {
  const double lo[3] = {-0.032, -0.034, -0.012}, hi[3] = {0.026, 0.020, 0.012};
  if (e < 12) {
    const int axis = e >> 2, b0 = e & 1, b1 = (e >> 1) & 1;
    // the two fixed coordinates, in rising order of their axis, take the bits b0 and b1
    const int bx = axis == 0 ? 0 : b0, by = axis == 0 ? b0 : (axis == 1 ? 0 : b1), bz = axis == 2 ? 0 : b1;
    a[0] = bx ? hi[0] : lo[0]; a[1] = by ? hi[1] : lo[1]; a[2] = bz ? hi[2] : lo[2];
    b[0] = a[0]; b[1] = a[1]; b[2] = a[2];
    if (axis == 0) b[0] = hi[0]; else if (axis == 1) b[1] = hi[1]; else b[2] = hi[2];
    return;
  }
  const int k = e - 12, n = (k + 1) & 3;
  const double h = 0.012;
  a[0] = (k == 1 || k == 2) ? h : -h; a[1] = (k >= 2) ? h : -h; a[2] = -0.017;
  b[0] = (n == 1 || n == 2) ? h : -h; b[1] = (n >= 2) ? h : -h; b[2] = -0.017;
}

// The glyph's rotation: toRotationMatrix(qWO), qWO = qWR * (0, 0, 1, 0) = (-qy, -qz, qw, qx), no normalisation
SL2_HD void world_glyph_rot(const double q[4], double R[9]) {
  const double qwo[4] = {-q[2], -q[3], q[0], q[1]};
  quat_to_rot(qwo, R);
}

// A glyph point in the world: W[i] = r[i] + ((0.0 + R[i][0] g[0]) + R[i][1] g[1]) + R[i][2] g[2]
SL2_HD void world_glyph_point(const double r[3], const double R[9], const double g[3], double W[3]) {
  for (int i = 0; i < 3; ++i) {
    double acc = 0.0;
    for (int k = 0; k < 3; ++k) acc += R[i * 3 + k] * g[k];
    W[i] = r[i] + acc;
  }
}

// The world segment A .. B through the view: both ends into the view frame, then the 3-D segment rule
SL2_HD bool world_segment(const sl2_view& v, const double xp[7], const double A[3], const double B[3], int out[4]) {
  double a[3], b[3];
  zeroedyi_only(xp, A, a);
  zeroedyi_only(xp, B, b);
  return scene_segment(v.fku, v.fkv, v.u0, v.v0, a, b, out);
}

// Glyph edge e of the camera at (r, q) of xv_, seen through the view
SL2_HD bool world_glyph_segment(const sl2_view& v, const double xp[7], const double xv[7], int e, int out[4]) {
  double R[9], ga[3], gb[3], A[3], B[3];
  world_glyph_rot(&xv[3], R);
  world_glyph_edge(e, ga, gb);
  world_glyph_point(xv, R, ga, A);
  world_glyph_point(xv, R, gb, B);
  return world_segment(v, xp, A, B, out);
}

// The extents (UpdateDrawingDimension), a coordinate at a time: v < min: min = v; v > max: max = v
SL2_HD void world_extend(double* lo, double* hi, double v) {
  if (v < *lo) *lo = v;
  if (v > *hi) *hi = v;
}

// Axis k (0 .. 2) from lo to hi, seen through the view
SL2_HD bool world_axis_segment(const sl2_view& v, const double xp[7], double lo, double hi, int k, int out[4]) {
  const double z = 0.0;
  const double A[3] = {k == 0 ? lo : z, k == 1 ? lo : z, k == 2 ? lo : z}, B[3] = {k == 0 ? hi : z, k == 1 ? hi : z, k == 2 ? hi : z};
  return world_segment(v, xp, A, B, out);
}

// The marker and the ring of a fully initialised feature at y with covariance block Pyy (read only where the ring is asked for)
SL2_HD void world_feature(const sl2_view& v, const double xp[7], const double y[3], const double* Pyy, bool want_marker, bool want_ring,
                          bool* has_marker, int mk[2], bool* has_ring, int rc[2], double q[4]) {
  double m[3], Jy[9];
  world_zeroed(xp, y, m, Jy);
  *has_marker = false; *has_ring = false;
  if (want_marker && m[2] >= kSceneNear) {
    double p[2];
    scene_project(v.fku, v.fkv, v.u0, v.v0, m, p);
    *has_marker = overlay_round(p[0], &mk[0]) && overlay_round(p[1], &mk[1]);
  }
  if (want_ring) {
    double Sg[9], centre[2];
    world_sigma(Jy, Pyy, Sg);
    *has_ring = scene_conic(v.fku, v.fkv, v.u0, v.v0, m, Sg, centre, q) && overlay_round(centre[0], &rc[0]) && overlay_round(centre[1], &rc[1]);
  }
}

// The ray of a partially initialised feature, y6 = r_i, hhat_i, in the world
SL2_HD bool world_ray(const sl2_view& v, const double xp[7], const double y6[6], int out[4]) {
  const double A[3] = {y6[0], y6[1], y6[2]};
  const double B[3] = {y6[0] + kSceneRayLength * y6[3], y6[1] + kSceneRayLength * y6[4], y6[2] + kSceneRayLength * y6[5]};
  return world_segment(v, xp, A, B, out);
}

// ---- picking: does the item cover a pixel of the window x0 .. x1, y0 .. y1 (inclusive, inside the image)?  Coverage is
// overlay_hit's; a PATCH covers its whole 13 x 13 box (its template is not looked at).
SL2_HD bool pick_item_hits(const sl2_overlay_item& it, int npatches, int x0, int y0, int x1, int y1) {
  if (it.label < 0) return false;
  OverlayPrep p;
  if (!overlay_prepare(it, npatches, &p) || !overlay_box_meets(p, x0, y0, x1, y1)) return false;
  if (p.kind == SL2_ITEM_PATCH) return true;      // the box is the square
  uint32_t rgb;
  for (int y = y0; y <= y1; ++y)
    for (int x = x0; x <= x1; ++x)
      if (overlay_hit(p, nullptr, 0, x, y, &rgb)) return true;
  return false;
}

// The window of a click, clipped; false: the click lies outside the image
SL2_HD bool pick_window(int width, int height, int x, int y, int* x0, int* y0, int* x1, int* y1) {
  if (x < 0 || y < 0 || x >= width || y >= height) return false;
  *x0 = x - 3 < 0 ? 0 : x - 3; *y0 = y - 3 < 0 ? 0 : y - 3;
  *x1 = x + 3 > width - 1 ? width - 1 : x + 3; *y1 = y + 3 > height - 1 ? height - 1 : y + 3;
  return true;
}

// The host form's body: one image
inline void pick_host_body(int width, int height, const sl2_overlay_item* items, int count, int npatches, int x, int y, int32_t picked[2]) {
  picked[0] = -1; picked[1] = -1;
  int x0, y0, x1, y1;
  if (!pick_window(width, height, x, y, &x0, &y0, &x1, &y1)) return;
  for (int k = count - 1; k >= 0; --k)
    if (pick_item_hits(items[k], npatches, x0, y0, x1, y1)) { picked[0] = items[k].label; picked[1] = k; return; }
}

}  // namespace sl2
