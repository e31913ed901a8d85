// Annotated frames: the pixel rules of a draw list - sl2_overlay_item, include/scenelib2_amd.h - as SL2_HD
// functions.  The same source is the body of k_overlay_draw (sl2_overlay.hip) and of sl2_draw_items_host, and a stand-alone host
// program can include it (tests/overlay_host.cpp): the two forms agree byte for byte by construction, given -ffp-contract=off.
//
// An item is PREPARED once (overlay_prepare: is it drawn at all, and a conservative box around what it covers) and then asked
// pixel by pixel (overlay_hit).  The box only ever skips work: what an item covers is decided by overlay_hit alone.
#pragma once
#include "../../include/scenelib2_amd.h"
#include "sl2_math.hpp"

namespace sl2 {

constexpr int kOverlayCoordMax = 32767;      // an item's centre lies within +-this (the list kernel omits the others)
constexpr int kOverlayMaxSide = 32768;       // image width and height at most
constexpr int kOverlayBoxHalfMax = 1 << 20;  // a ring's box is cut here: beyond any image around any centre

struct OverlayPrep {      // 72 bytes
  int kind;               // SL2_ITEM_*
  int cx, cy;             // RING, PATCH: the centre
  int bx0, by0, bx1, by1; // conservative inclusive box (RECT: the rectangle itself; SEGMENT: the endpoints' box)
  int patch;
  uint32_t rgb;           // r | g << 8 | b << 16
  int pad;                // SEGMENT: kSegYMajor | kSegMinorFalls (the box holds the rest: its sides are |dx| and |dy|); else 0
  double A, B, C, rhs;
};

constexpr int kSegYMajor = 1;      // |dy| > |dx|: y is the major coordinate
constexpr int kSegMinorFalls = 2;  // walking the major coordinate upwards, the minor one decreases

SL2_HD bool overlay_finite(double v) { return v - v == 0.0; }

// inside(du, dv) of the header, in its order: ((A du) du + (B du) dv) + (C dv) dv < rhs
SL2_HD bool overlay_inside(double A, double B, double C, double rhs, int du, int dv) {
  const double x = (double)du, y = (double)dv;
  return ((A * x) * x + (B * x) * y) + (C * y) * y < rhs;
}

SL2_HD bool overlay_ring_valid(const double q[4]) {
  if (!(overlay_finite(q[0]) && overlay_finite(q[1]) && overlay_finite(q[2]) && overlay_finite(q[3]))) return false;
  return q[0] > 0.0 && q[2] > 0.0 && (4.0 * q[0]) * q[2] - q[1] * q[1] > 0.0 && q[3] > 0.0;
}

// Half-extents of a box that holds every (du, dv) with inside(du, dv): the ellipse reaches |du| <= sqrt(4 C rhs / det) and
// |dv| <= sqrt(4 A rhs / det), det = 4 A C - B^2.  det is taken at the low end of what its rounding allows (where that is not
// positive the box is everything), and the extents get a relative and an absolute margin that dwarf inside()'s own rounding.
SL2_HD void overlay_ring_half(double A, double B, double C, double rhs, int* hx, int* hy) {
  const double ac = (4.0 * A) * C, bb = B * B;
  const double det = (ac - bb) - 1e-15 * (ac + bb);
  *hx = kOverlayBoxHalfMax; *hy = kOverlayBoxHalfMax;
  if (!(det > 0.0)) return;
  const double ex = sqrt((4.0 * C) * rhs / det) * (1.0 + 1e-9) + 2.0;
  const double ey = sqrt((4.0 * A) * rhs / det) * (1.0 + 1e-9) + 2.0;
  if (ex < (double)kOverlayBoxHalfMax) *hx = (int)ex + 1;
  if (ey < (double)kOverlayBoxHalfMax) *hy = (int)ey + 1;
}

SL2_HD int overlay_clampc(int v) { return v < -kOverlayBoxHalfMax ? -kOverlayBoxHalfMax : v > kOverlayBoxHalfMax ? kOverlayBoxHalfMax : v; }

// SEGMENT, the header's rule with the division multiplied out: with t = major - major0 in [0, D], d = the signed minor extent and
// k = minor - minor0, k == floor((2 t d + D) / (2 D)) iff 2 D k <= 2 t d + D < 2 D k + 2 D.  All in 64-bit integers: the
// coordinates are clamped to +-2^20, so D, |d| <= 2^21, |k| <= 2^21 and no product passes 2^44.  D == 0: the single pixel.
SL2_HD bool overlay_segment_covers(int D, int d, int t, int k) {
  if (D == 0) return t == 0 && k == 0;
  const long long n = 2ll * t * d + D, lo = 2ll * D * k;
  return lo <= n && n < lo + 2ll * D;
}

// False: the item draws nothing (unknown kind, patch index outside the array, invalid ring, inverted rectangle).
SL2_HD bool overlay_prepare(const sl2_overlay_item& it, int npatches, OverlayPrep* p) {
  p->kind = it.kind;
  p->rgb = (uint32_t)it.rgb[0] | ((uint32_t)it.rgb[1] << 8) | ((uint32_t)it.rgb[2] << 16);
  p->patch = it.patch; p->pad = 0;
  p->A = it.q[0]; p->B = it.q[1]; p->C = it.q[2]; p->rhs = it.q[3];
  // Coordinates beyond +-2^20 (no image reaches 2^15): a rectangle's corners are pulled in, which clips the same; a ring or a
  // patch centred out there draws nothing (the header says so) - so that no sum below leaves the ints.
  const int a0 = overlay_clampc(it.a[0]), a1 = overlay_clampc(it.a[1]), a2 = overlay_clampc(it.a[2]), a3 = overlay_clampc(it.a[3]);
  p->cx = a0; p->cy = a1;
  p->bx0 = p->by0 = 0; p->bx1 = p->by1 = -1;
  if (it.kind == SL2_ITEM_SEGMENT) {      // (its ends are pulled in like a rectangle's corners)
    const int dx = a2 - a0, dy = a3 - a1, adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
    const bool ymajor = adx < ady;
    // the ends swapped so that the major coordinate does not decrease: the minor one falls iff the two differences differ in sign
    const bool falls = ymajor ? (dy < 0 ? dx > 0 : dx < 0) : (dx < 0 ? dy > 0 : dy < 0);
    p->pad = (ymajor ? kSegYMajor : 0) | (falls ? kSegMinorFalls : 0);
    p->bx0 = a0 < a2 ? a0 : a2; p->bx1 = a0 < a2 ? a2 : a0; p->by0 = a1 < a3 ? a1 : a3; p->by1 = a1 < a3 ? a3 : a1;
    return true;
  }
  if (it.kind != SL2_ITEM_RECT && (a0 != it.a[0] || a1 != it.a[1])) return false;
  if (it.kind == SL2_ITEM_RING) {
    if (!overlay_ring_valid(it.q)) return false;
    int hx, hy;
    overlay_ring_half(p->A, p->B, p->C, p->rhs, &hx, &hy);
    p->bx0 = a0 - hx; p->bx1 = a0 + hx; p->by0 = a1 - hy; p->by1 = a1 + hy;
    return true;
  }
  if (it.kind == SL2_ITEM_PATCH) {
    if (it.patch < 0 || it.patch >= npatches) return false;
    p->bx0 = a0 - 6; p->bx1 = a0 + 6; p->by0 = a1 - 6; p->by1 = a1 + 6;
    return true;
  }
  if (it.kind == SL2_ITEM_RECT) {
    if (a0 > a2 || a1 > a3) return false;
    p->bx0 = a0; p->by0 = a1; p->bx1 = a2; p->by1 = a3;
    return true;
  }
  return false;
}

SL2_HD bool overlay_box_meets(const OverlayPrep& p, int x0, int y0, int x1, int y1) {
  return p.bx0 <= x1 && p.bx1 >= x0 && p.by0 <= y1 && p.by1 >= y0;
}

// Does the prepared item cover pixel (x, y), and with which colour (r | g << 8 | b << 16)?
SL2_HD bool overlay_hit(const OverlayPrep& p, const uint8_t* patches, size_t patch_stride, int x, int y, uint32_t* rgb) {
  if (x < p.bx0 || x > p.bx1 || y < p.by0 || y > p.by1) return false;
  if (p.kind == SL2_ITEM_RING) {
    const int du = x - p.cx, dv = y - p.cy;
    if (!overlay_inside(p.A, p.B, p.C, p.rhs, du, dv)) return false;
    if (overlay_inside(p.A, p.B, p.C, p.rhs, du - 1, dv) && overlay_inside(p.A, p.B, p.C, p.rhs, du + 1, dv) &&
        overlay_inside(p.A, p.B, p.C, p.rhs, du, dv - 1) && overlay_inside(p.A, p.B, p.C, p.rhs, du, dv + 1))
      return false;
    *rgb = p.rgb;
    return true;
  }
  if (p.kind == SL2_ITEM_PATCH) {
    const int du = x - p.cx, dv = y - p.cy;      // |du|, |dv| <= 6: the box
    if (du >= -5 && du <= 5 && dv >= -5 && dv <= 5) {
      const uint32_t g = patches[(size_t)p.patch * patch_stride + (size_t)((dv + 5) * 11 + du + 5)];
      *rgb = g | (g << 8) | (g << 16);
    } else {
      *rgb = p.rgb;
    }
    return true;
  }
  if (p.kind == SL2_ITEM_SEGMENT) {
    const int W = p.bx1 - p.bx0, H = p.by1 - p.by0;      // |dx|, |dy|
    const bool falls = (p.pad & kSegMinorFalls) != 0;
    const bool on = (p.pad & kSegYMajor) ? overlay_segment_covers(H, falls ? -W : W, y - p.by0, x - (falls ? p.bx1 : p.bx0))
                                         : overlay_segment_covers(W, falls ? -H : H, x - p.bx0, y - (falls ? p.by1 : p.by0));
    if (!on) return false;
    *rgb = p.rgb;
    return true;
  }
  // RECT: the outline of the box
  if (x != p.bx0 && x != p.bx1 && y != p.by0 && y != p.by1) return false;
  *rgb = p.rgb;
  return true;
}

// Why a list cannot be drawn (nullptr: it can): the checks the host makes of a host-resident list.
inline const char* overlay_item_fault(const sl2_overlay_item& it, int npatches) {
  if (it.kind != SL2_ITEM_RING && it.kind != SL2_ITEM_PATCH && it.kind != SL2_ITEM_RECT && it.kind != SL2_ITEM_SEGMENT) return "unknown item kind";
  if (it.kind == SL2_ITEM_PATCH && (it.patch < 0 || it.patch >= npatches)) return "patch index outside the patches array";
  return nullptr;
}

// The host form's body: one image.  prep: scratch of `count` records.
inline void overlay_draw_host_body(const uint8_t* frame, int width, int height, const sl2_overlay_item* items, int count, const uint8_t* patches,
                                   size_t patch_stride, int npatches, OverlayPrep* prep, uint8_t* out) {
  int n = 0;
  for (int k = 0; k < count; ++k)
    if (overlay_prepare(items[k], npatches, &prep[n]) && overlay_box_meets(prep[n], 0, 0, width - 1, height - 1)) ++n;
  for (int y = 0; y < height; ++y)
    for (int x = 0; x < width; ++x) {
      const uint32_t g = frame[(size_t)y * width + x];
      uint32_t c = g | (g << 8) | (g << 16), h;
      for (int k = 0; k < n; ++k)
        if (overlay_hit(prep[k], patches, patch_stride, x, y, &h)) c = h;
      uint8_t* o = out + ((size_t)y * width + x) * 3;
      o[0] = (uint8_t)c; o[1] = (uint8_t)(c >> 8); o[2] = (uint8_t)(c >> 16);
    }
}

// ---- the draw list of a sequence: the pieces the list kernel and the header's words share

// int(v + 0.5) as C truncates it; false where v is not finite or the result lies outside +-kOverlayCoordMax (the item is omitted)
SL2_HD bool overlay_round(double v, int* out) {
  if (!(v > -40000.0 && v < 40000.0)) return false;
  const int c = (int)(v + 0.5);
  if (c < -kOverlayCoordMax || c > kOverlayCoordMax) return false;
  *out = c;
  return true;
}

// The reference's particle counter (graphictool.cpp:716-733): of n particles, particle k (from 0) is drawn iff (k + 1) % step == 0
SL2_HD int overlay_particle_step(int n) { const int s = n / 10; return s > 1 ? s : 1; }

SL2_HD void overlay_colour(bool marked, bool selected, bool matched, uint8_t rgb[3]) {
  if (marked) { rgb[0] = 0; rgb[1] = 255; rgb[2] = 0; }
  else if (selected && matched) { rgb[0] = 255; rgb[1] = 0; rgb[2] = 0; }
  else if (selected) { rgb[0] = 0; rgb[1] = 0; rgb[2] = 255; }
  else { rgb[0] = 255; rgb[1] = 255; rgb[2] = 0; }
}

SL2_HD sl2_overlay_item overlay_blank_item(int kind, int label) {
  sl2_overlay_item it;
  it.kind = kind; it.label = label;
  it.a[0] = it.a[1] = it.a[2] = it.a[3] = 0;
  it.patch = -1;
  it.rgb[0] = it.rgb[1] = it.rgb[2] = 0; it.pad = 0;
  it.q[0] = it.q[1] = it.q[2] = it.q[3] = 0.0;
  return it;
}

}  // namespace sl2
