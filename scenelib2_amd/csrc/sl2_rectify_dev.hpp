// The undistorted frame: the pixel rule of sl2_rectify_frames - include/scenelib2_amd.h, "the rectified
// view" - as SL2_HD functions.  The same source is the body of k_rectify (sl2_rectify.hip) and of sl2_rectify_frame_host, and a
// stand-alone host program can include it (tests/rectified_host.cpp): the two forms agree byte for byte by construction, given
// -ffp-contract=off and a correctly rounded FP64 square root and division on both sides.
#pragma once
#include "../../include/scenelib2_amd.h"
#include "sl2_math.hpp"

namespace sl2 {

constexpr int kRectifyMaxSide = 32768;               // image width and height at most
constexpr double kRectifySourceMax = 1048576.0;      // a source position beyond +-2^20 is the border (so that 32 xs fits an int)
constexpr int kRectifyBorder = 0;

// A tap: the source pixel, or the border off the image
SL2_HD int rectify_tap(const uint8_t* __restrict__ src, int width, int height, int x, int y) {
  return (x >= 0 && x < width && y >= 0 && y < height) ? (int)src[(size_t)y * width + x] : kRectifyBorder;
}

// Where output pixel (x, y) reads the source, in 1/32 pixel; false: the border.  The header's expressions, in its order.
SL2_HD bool rectify_source(double u0, double v0, double kd1, int x, int y, int* X, int* Y) {
  const double cx = (double)x - u0, cy = (double)y - v0;
  const double r2 = cx * cx + cy * cy;
  const double f = 1.0 + (2.0 * kd1) * r2;
  if (!(f > 0.0)) return false;
  const double s = sqrt(f);
  const double xs = cx / s + u0, ys = cy / s + v0;
  // (a NaN or an infinity fails one of the four comparisons)
  if (!(xs >= -kRectifySourceMax && xs <= kRectifySourceMax && ys >= -kRectifySourceMax && ys <= kRectifySourceMax)) return false;
  *X = (int)floor(xs * 32.0 + 0.5);
  *Y = (int)floor(ys * 32.0 + 0.5);
  return true;
}

SL2_HD uint8_t rectify_pixel(const uint8_t* __restrict__ src, int width, int height, double u0, double v0, double kd1, int x, int y) {
  int X, Y;
  if (!rectify_source(u0, v0, kd1, x, y, &X, &Y)) return (uint8_t)kRectifyBorder;
  const int fx = X & 31, fy = Y & 31;                  // (two's complement: 0 .. 31 for a negative X too)
  const int ix = (X - fx) / 32, iy = (Y - fy) / 32;    // X >> 5 floored: X - fx is a multiple of 32
  // The weights of an absent neighbour are 0 when fx or fy is: it is not read then (an image's last column maps onto itself
  // with kd1 == 0 without a tap beyond it; the value is the same either way)
  const int p00 = rectify_tap(src, width, height, ix, iy);
  const int p10 = fx ? rectify_tap(src, width, height, ix + 1, iy) : 0;
  const int p01 = fy ? rectify_tap(src, width, height, ix, iy + 1) : 0;
  const int p11 = (fx && fy) ? rectify_tap(src, width, height, ix + 1, iy + 1) : 0;
  return (uint8_t)(((32 - fx) * (32 - fy) * p00 + fx * (32 - fy) * p10 + (32 - fx) * fy * p01 + fx * fy * p11 + 512) >> 10);
}

// The host form's body: one image
inline void rectify_host_body(const uint8_t* frame, int width, int height, double u0, double v0, double kd1, uint8_t* out) {
  for (int y = 0; y < height; ++y)
    for (int x = 0; x < width; ++x) out[(size_t)y * width + x] = rectify_pixel(frame, width, height, u0, v0, kd1, x, y);
}

// ---- the 3-D scene in the rectified image (sl2_scene_items): the pieces k_scene_list and the header's words share.  The
// camera of the rectified image is the sequence's with kd1 = 0.

constexpr double kSceneNear = 0.01;           // kNear_ (graphictool.cpp): what lies nearer the camera plane is not drawn
constexpr double kSceneRayLength = 10.0;      // kSemiInfiniteLineLength_
constexpr double kSceneGuard = 32767.0;       // = kOverlayCoordMax: the square a projected segment is clipped to

// func_zeroedyi_and_dzeroedyi_by_dxp_and_dzeroedyi_by_dyi (full_feature_model.cpp:67-101), the expressions of
// measurement_model (sl2_math.hpp): m = RRW (y - r), Jx = dzeroedyi_by_dxp (3x7 row-major), Jy = dzeroedyi_by_dyi = RRW (3x3)
SL2_HD void scene_zeroed_jac(const double xp[7], const double y[3], double m[3], double Jx[21], double Jy[9]) {
  const double d[3] = {y[0] - xp[0], y[1] - xp[1], y[2] - xp[2]};
  double qRW[4];
  quat_inverse(&xp[3], qRW);
  quat_to_rot(qRW, Jy);
  for (int i = 0; i < 3; ++i) {
    double acc = 0.0;
    for (int k = 0; k < 3; ++k) acc += Jy[i * 3 + k] * d[k];
    m[i] = acc;
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Jx[i * 7 + j] = Jy[i * 3 + j] * -1.0;
  const double w = qRW[0], x = qRW[1], yy = qRW[2], z = qRW[3];
  const double t[4][9] = {{2 * w, -2 * z, 2 * yy, 2 * z, 2 * w, -2 * x, -2 * yy, 2 * x, 2 * w},
                          {2 * x, 2 * yy, 2 * z, 2 * yy, -2 * x, -2 * w, 2 * z, 2 * w, -2 * x},
                          {-2 * yy, 2 * x, 2 * w, 2 * x, 2 * yy, 2 * z, -2 * w, 2 * z, -2 * yy},
                          {-2 * z, -2 * w, 2 * x, 2 * w, -2 * z, 2 * yy, 2 * x, 2 * yy, 2 * z}};
  for (int k = 0; k < 4; ++k) {
    const double sgn = (k == 0) ? 1.0 : -1.0;
    for (int i = 0; i < 3; ++i) {
      double acc = 0.0;
      for (int c = 0; c < 3; ++c) acc += t[k][i * 3 + c] * d[c];
      Jx[i * 7 + 3 + k] = acc * sgn;
    }
  }
}

// Pzeroedyigraphics (feature_model.cpp:128-145; dxp_by_dxv is the identity on the first seven columns, so the sums are
// 7-wide), in the header's order: every inner sum starts at 0.0 and runs upwards;
// Sg[i][j] = ((T1[i][j] + T3[j][i]) + T3[i][j]) + T4[i][j], T1 = (Jx Pxx) Jx^T, T3 = (Jx Pxy) Jy^T, T4 = (Jy Pyy) Jy^T.
SL2_HD void scene_sigma(const double Jx[21], const double Jy[9], const double Pxx7[49], const double Pxy7[21], const double Pyy[9], double Sg[9]) {
  double A[21], B[9], C[9], T3[9];
  for (int i = 0; i < 3; ++i) {
    for (int c = 0; c < 7; ++c) {
      double acc = 0.0;
      for (int k = 0; k < 7; ++k) acc += Jx[i * 7 + k] * Pxx7[k * 7 + c];
      A[i * 7 + c] = acc;
    }
    for (int c = 0; c < 3; ++c) {
      double acc = 0.0;
      for (int k = 0; k < 7; ++k) acc += Jx[i * 7 + k] * Pxy7[k * 3 + c];
      B[i * 3 + c] = acc;
      double acc2 = 0.0;
      for (int k = 0; k < 3; ++k) acc2 += Jy[i * 3 + k] * Pyy[k * 3 + c];
      C[i * 3 + c] = acc2;
    }
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double acc = 0.0;
      for (int c = 0; c < 3; ++c) acc += B[i * 3 + c] * Jy[j * 3 + c];
      T3[i * 3 + j] = acc;
    }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double t1 = 0.0, t4 = 0.0;
      for (int c = 0; c < 7; ++c) t1 += A[i * 7 + c] * Jx[j * 7 + c];
      for (int c = 0; c < 3; ++c) t4 += C[i * 3 + c] * Jy[j * 3 + c];
      Sg[i * 3 + j] = ((t1 + T3[j * 3 + i]) + T3[i * 3 + j]) + t4;
    }
}

// The outline of the 3-sigma ellipsoid (X - m)^T Sg^-1 (X - m) = 9 under the pinhole: the dual conic D = m m^T - 9 Sg.
// False: d = D22 is not positive (the ellipsoid reaches the camera plane) or m[2] is not (d > 0 holds for an ellipsoid wholly
// BEHIND the plane too) - no item.  centre: unrounded; q: A, B, C, rhs.
SL2_HD bool scene_conic(double fku, double fkv, double u0, double v0, const double m[3], const double Sg[9], double centre[2], double q[4]) {
  const double D00 = m[0] * m[0] - 9.0 * Sg[0], D01 = m[0] * m[1] - 9.0 * Sg[1], D02 = m[0] * m[2] - 9.0 * Sg[2];
  const double D11 = m[1] * m[1] - 9.0 * Sg[4], D12 = m[1] * m[2] - 9.0 * Sg[5], d = m[2] * m[2] - 9.0 * Sg[8];
  if (!(d > 0.0 && m[2] > 0.0)) return false;
  const double cn0 = D02 / d, cn1 = D12 / d;
  const double En00 = cn0 * cn0 - D00 / d, En01 = cn0 * cn1 - D01 / d, En11 = cn1 * cn1 - D11 / d;
  const double E00 = (fku * En00) * fku, E01 = (fku * En01) * fkv, E11 = (fkv * En11) * fkv;
  centre[0] = u0 - fku * cn0; centre[1] = v0 - fkv * cn1;
  q[0] = E11; q[1] = -2.0 * E01; q[2] = E00; q[3] = E00 * E11 - E01 * E01;
  return true;
}

// A camera-frame point in front of the near plane, in the rectified image (unrounded)
SL2_HD void scene_project(double fku, double fkv, double u0, double v0, const double X[3], double p[2]) {
  p[0] = u0 - fku * X[0] / X[2];
  p[1] = v0 - fkv * X[1] / X[2];
}

// A 3-D segment a .. b of the camera frame as a SEGMENT's four coordinates, in the header's order: clip to X[2] >= kSceneNear
// (an end behind moves along the segment onto the plane, its X[2] set to kSceneNear exactly), project both ends, clip the 2-D
// segment to the guard square (Liang-Barsky), round.  False: entirely behind, entirely outside, or not finite - no item.
SL2_HD bool scene_segment(double fku, double fkv, double u0, double v0, const double a_in[3], const double b_in[3], int out[4]) {
  double a[3] = {a_in[0], a_in[1], a_in[2]}, b[3] = {b_in[0], b_in[1], b_in[2]};
  const bool a_behind = !(a[2] >= kSceneNear), b_behind = !(b[2] >= kSceneNear);
  if (a_behind && b_behind) return false;
  if (a_behind || b_behind) {
    const double t = (kSceneNear - a[2]) / (b[2] - a[2]);      // from a towards b, in (0, 1]
    const double cx = a[0] + t * (b[0] - a[0]), cy = a[1] + t * (b[1] - a[1]);
    if (a_behind) { a[0] = cx; a[1] = cy; a[2] = kSceneNear; } else { b[0] = cx; b[1] = cy; b[2] = kSceneNear; }
  }
  double p[2], r[2];
  scene_project(fku, fkv, u0, v0, a, p);
  scene_project(fku, fkv, u0, v0, b, r);
  if (!(overlay_finite(p[0]) && overlay_finite(p[1]) && overlay_finite(r[0]) && overlay_finite(r[1]))) return false;
  const double dx = r[0] - p[0], dy = r[1] - p[1];
  double t0 = 0.0, t1 = 1.0;
  // the four edges in the order left, right, top, bottom: pk t <= qk
  const double pk[4] = {-dx, dx, -dy, dy}, qk[4] = {p[0] + kSceneGuard, kSceneGuard - p[0], p[1] + kSceneGuard, kSceneGuard - p[1]};
  for (int k = 0; k < 4; ++k) {
    if (pk[k] == 0.0) { if (qk[k] < 0.0) return false; continue; }
    const double t = qk[k] / pk[k];
    if (pk[k] < 0.0) { if (t > t1) return false; if (t > t0) t0 = t; }
    else { if (t < t0) return false; if (t < t1) t1 = t; }
  }
  const double ax = p[0] + t0 * dx, ay = p[1] + t0 * dy, bx = p[0] + t1 * dx, by = p[1] + t1 * dy;
  return overlay_round(ax, &out[0]) && overlay_round(ay, &out[1]) && overlay_round(bx, &out[2]) && overlay_round(by, &out[3]);
}

}  // namespace sl2
