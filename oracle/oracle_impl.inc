/* oracle_impl.inc — TEST INFRASTRUCTURE ONLY.  Included twice by tvmi_oracle.c with
 * REAL = float / double and FN(x) = x##_f32 / x##_f64.  Plain scalar C restatement of the
 * reference CPU algorithms; every function cites the reference lines it follows
 * (paths relative to torchvision/csrc/ops/).  Built with -O2 -ffp-contract=off for the
 * x86-64 baseline (no FMA), i.e. the arithmetic of the reference's own CPU build.
 */

/* ---- cpu/nms_kernel.cpp:17-95.  order = stable descending argsort of scores (done by the
 * caller exactly like aten::sort(stable=True, descending=True)).  Returns #kept. */
int64_t FN(oracle_nms)(const REAL* dets, const int64_t* order, const int64_t* seg, int64_t n, double thr,
                       int64_t* keep) {
  unsigned char* suppressed = (unsigned char*)calloc((size_t)(n > 0 ? n : 1), 1);
  REAL* areas = (REAL*)malloc(sizeof(REAL) * (size_t)(n > 0 ? n : 1));
  for (int64_t k = 0; k < n; ++k) areas[k] = (dets[4 * k + 2] - dets[4 * k + 0]) * (dets[4 * k + 3] - dets[4 * k + 1]);
  int64_t kept = 0;
  for (int64_t a = 0; a < n; ++a) {
    const int64_t i = order[a];
    if (suppressed[i]) continue;
    keep[kept++] = i;
    const REAL ix1 = dets[4 * i], iy1 = dets[4 * i + 1], ix2 = dets[4 * i + 2], iy2 = dets[4 * i + 3];
    const REAL iarea = areas[i];
    for (int64_t b = a + 1; b < n; ++b) {
      const int64_t j = order[b];
      if (suppressed[j]) continue;
      if (seg && seg[i] != seg[j]) continue; /* batched form: ops/boxes.py:113-126 */
      const REAL xx1 = ix1 > dets[4 * j] ? ix1 : dets[4 * j];
      const REAL yy1 = iy1 > dets[4 * j + 1] ? iy1 : dets[4 * j + 1];
      const REAL xx2 = dets[4 * j + 2] < ix2 ? dets[4 * j + 2] : ix2;
      const REAL yy2 = dets[4 * j + 3] < iy2 ? dets[4 * j + 3] : iy2;
      const REAL dw = xx2 - xx1, dh = yy2 - yy1;
      const REAL w = (REAL)0 < dw ? dw : (REAL)0, h = (REAL)0 < dh ? dh : (REAL)0;
      const REAL inter = w * h;
      const REAL ovr = inter / (iarea + areas[j] - inter);
      if ((double)ovr > thr) suppressed[j] = 1;
    }
  }
  free(suppressed);
  free(areas);
  return kept;
}

/* ---- shared bilinear set-up of the RoIAlign family:
 * cpu/roi_align_common.h:50-103 == cpu/roi_align_kernel.cpp:117-176 == cpu/ps_roi_align_kernel.cpp:17-70 */
static int FN(bilin)(int H, int W, REAL y, REAL x, int* yl, int* yh, int* xl, int* xh, REAL* w1, REAL* w2, REAL* w3,
                     REAL* w4) {
  if (y < -1.0 || y > H || x < -1.0 || x > W) return 0;
  if (y <= 0) y = 0;
  if (x <= 0) x = 0;
  *yl = (int)y;
  *xl = (int)x;
  if (*yl >= H - 1) {
    *yh = *yl = H - 1;
    y = (REAL)*yl;
  } else {
    *yh = *yl + 1;
  }
  if (*xl >= W - 1) {
    *xh = *xl = W - 1;
    x = (REAL)*xl;
  } else {
    *xh = *xl + 1;
  }
  const REAL ly = y - *yl, lx = x - *xl;
  const REAL hy = (REAL)(1. - ly), hx = (REAL)(1. - lx);
  *w1 = hy * hx;
  *w2 = hy * lx;
  *w3 = ly * hx;
  *w4 = ly * lx;
  return 1;
}

/* ---- cpu/roi_align_kernel.cpp:18-115 (forward) and :183-289 (backward, `backward` != 0:
 * `data` is grad_output [K,C,PH,PW] contiguous and `out` is grad_input, pre-zeroed). */
void FN(oracle_roi_align)(const REAL* data, const REAL* rois, REAL* out, int K, int C, int H, int W, int PH, int PW,
                          double spatial_scale, int sampling_ratio, int aligned, int backward) {
  const REAL scale = (REAL)spatial_scale;
  for (int n = 0; n < K; ++n) {
    const REAL* r = rois + 5 * n;
    const int b = (int)r[0];
    const REAL off = aligned ? (REAL)0.5 : (REAL)0.0;
    const REAL sw = r[1] * scale - off, sh = r[2] * scale - off;
    const REAL ew = r[3] * scale - off, eh = r[4] * scale - off;
    REAL rw = ew - sw, rh = eh - sh;
    if (!aligned) {
      rw = rw > (REAL)1. ? rw : (REAL)1.;
      rh = rh > (REAL)1. ? rh : (REAL)1.;
    }
    const REAL bin_h = rh / (REAL)PH, bin_w = rw / (REAL)PW;
    const int gh = sampling_ratio > 0 ? sampling_ratio : (int)ceil(rh / PH);
    const int gw = sampling_ratio > 0 ? sampling_ratio : (int)ceil(rw / PW);
    const int cnt = gh * gw;
    const REAL count_f = (REAL)(cnt > 1 ? cnt : 1); /* forward: max(gh*gw, 1) */
    const REAL count_b = (REAL)cnt;                 /* backward: gh*gw */
    for (int c = 0; c < C; ++c) {
      const size_t plane = ((size_t)b * C + c) * H * W;
      for (int ph = 0; ph < PH; ++ph)
        for (int pw = 0; pw < PW; ++pw) {
          const size_t oidx = (((size_t)n * C + c) * PH + ph) * PW + pw;
          REAL acc = 0;
          for (int iy = 0; iy < gh; ++iy) {
            const REAL y = sh + ph * bin_h + (REAL)(iy + .5f) * bin_h / (REAL)gh;
            for (int ix = 0; ix < gw; ++ix) {
              const REAL x = sw + pw * bin_w + (REAL)(ix + .5f) * bin_w / (REAL)gw;
              int yl, yh, xl, xh;
              REAL w1, w2, w3, w4;
              if (!FN(bilin)(H, W, y, x, &yl, &yh, &xl, &xh, &w1, &w2, &w3, &w4)) continue;
              if (backward) {
                const REAL g = data[oidx];
                out[plane + (size_t)yl * W + xl] += g * w1 / count_b;
                out[plane + (size_t)yl * W + xh] += g * w2 / count_b;
                out[plane + (size_t)yh * W + xl] += g * w3 / count_b;
                out[plane + (size_t)yh * W + xh] += g * w4 / count_b;
              } else {
                acc += w1 * data[plane + (size_t)yl * W + xl] + w2 * data[plane + (size_t)yl * W + xh] +
                       w3 * data[plane + (size_t)yh * W + xl] + w4 * data[plane + (size_t)yh * W + xh];
              }
            }
          }
          if (!backward) out[oidx] = acc / count_f;
        }
    }
  }
}

/* ---- cpu/roi_pool_kernel.cpp:24-91 (forward; argmax int32) */
void FN(oracle_roi_pool)(const REAL* in, const REAL* rois, REAL* out, int32_t* argmax, int K, int C, int H, int W,
                         int PH, int PW, double spatial_scale) {
  const REAL scale = (REAL)spatial_scale;
  for (int n = 0; n < K; ++n) {
    const REAL* r = rois + 5 * n;
    const int b = (int)r[0];
    const int rsw = (int)round(r[1] * scale), rsh = (int)round(r[2] * scale);
    const int rew = (int)round(r[3] * scale), reh = (int)round(r[4] * scale);
    const int rw = (rew - rsw + 1) > 1 ? (rew - rsw + 1) : 1, rh = (reh - rsh + 1) > 1 ? (reh - rsh + 1) : 1;
    const REAL bin_h = (REAL)rh / (REAL)PH, bin_w = (REAL)rw / (REAL)PW;
    for (int ph = 0; ph < PH; ++ph)
      for (int pw = 0; pw < PW; ++pw) {
        int hs = (int)floor((REAL)ph * bin_h), ws = (int)floor((REAL)pw * bin_w);
        int he = (int)ceil((REAL)(ph + 1) * bin_h), we = (int)ceil((REAL)(pw + 1) * bin_w);
        hs = hs + rsh < 0 ? 0 : (hs + rsh > H ? H : hs + rsh);
        he = he + rsh < 0 ? 0 : (he + rsh > H ? H : he + rsh);
        ws = ws + rsw < 0 ? 0 : (ws + rsw > W ? W : ws + rsw);
        we = we + rsw < 0 ? 0 : (we + rsw > W ? W : we + rsw);
        const int empty = (he <= hs) || (we <= ws);
        for (int c = 0; c < C; ++c) {
          REAL maxval = empty ? 0 : -FLT_MAX;
          int maxidx = -1;
          const REAL* p = in + ((size_t)b * C + c) * H * W;
          for (int h = hs; h < he; ++h)
            for (int w = ws; w < we; ++w)
              if (p[h * W + w] > maxval) {
                maxval = p[h * W + w];
                maxidx = h * W + w;
              }
          const size_t o = (((size_t)n * C + c) * PH + ph) * PW + pw;
          out[o] = maxval;
          argmax[o] = maxidx;
        }
      }
  }
}

/* ---- cpu/roi_pool_kernel.cpp:93-134 (backward through argmax; grad contiguous) */
void FN(oracle_roi_pool_bwd)(const REAL* grad, const REAL* rois, const int32_t* argmax, REAL* gin, int K, int C, int H,
                             int W, int PH, int PW) {
  for (int n = 0; n < K; ++n) {
    const int b = (int)rois[5 * n];
    for (int c = 0; c < C; ++c)
      for (int i = 0; i < PH * PW; ++i) {
        const size_t o = ((size_t)n * C + c) * PH * PW + i;
        if (argmax[o] != -1) gin[((size_t)b * C + c) * H * W + argmax[o]] += grad[o];
      }
  }
}

/* ---- cpu/ps_roi_align_kernel.cpp:73-151 (forward) / :219-313 (backward) */
void FN(oracle_ps_roi_align)(const REAL* data, const REAL* rois, REAL* out, int32_t* mapping, int K, int C, int H,
                             int W, int PH, int PW, double spatial_scale, int sampling_ratio, int backward) {
  const REAL scale = (REAL)spatial_scale;
  const int C_out = C / (PH * PW);
  for (int n = 0; n < K; ++n) {
    const REAL* r = rois + 5 * n;
    const int b = (int)r[0];
    const REAL sw = r[1] * scale - (REAL)0.5, sh = r[2] * scale - (REAL)0.5;
    const REAL ew = r[3] * scale - (REAL)0.5, eh = r[4] * scale - (REAL)0.5;
    const REAL rw = ew - sw, rh = eh - sh;
    const REAL bin_h = rh / (REAL)PH, bin_w = rw / (REAL)PW;
    for (int co = 0; co < C_out; ++co)
      for (int ph = 0; ph < PH; ++ph)
        for (int pw = 0; pw < PW; ++pw) {
          const size_t o = (((size_t)n * C_out + co) * PH + ph) * PW + pw;
          const int c_in = backward ? mapping[o] : (co * PH + ph) * PW + pw;
          const REAL hstart = (REAL)ph * bin_h + sh, wstart = (REAL)pw * bin_w + sw;
          const int gh = sampling_ratio > 0 ? sampling_ratio : (int)ceil(rh / PH);
          const int gw = sampling_ratio > 0 ? sampling_ratio : (int)ceil(rw / PW);
          const REAL count = (REAL)(gh * gw);
          const size_t plane = ((size_t)b * C + c_in) * H * W;
          REAL sum = 0;
          for (int iy = 0; iy < gh; ++iy) {
            const REAL y = hstart + (REAL)(iy + .5f) * bin_h / (REAL)gh;
            for (int ix = 0; ix < gw; ++ix) {
              const REAL x = wstart + (REAL)(ix + .5f) * bin_w / (REAL)gw;
              int yl, yh, xl, xh;
              REAL w1, w2, w3, w4;
              if (!FN(bilin)(H, W, y, x, &yl, &yh, &xl, &xh, &w1, &w2, &w3, &w4)) continue;
              if (backward) {
                const REAL g = data[o];
                out[plane + (size_t)yl * W + xl] += g * w1 / count;
                out[plane + (size_t)yl * W + xh] += g * w2 / count;
                out[plane + (size_t)yh * W + xl] += g * w3 / count;
                out[plane + (size_t)yh * W + xh] += g * w4 / count;
              } else {
                sum += w1 * data[plane + (size_t)yl * W + xl] + w2 * data[plane + (size_t)yl * W + xh] +
                       w3 * data[plane + (size_t)yh * W + xl] + w4 * data[plane + (size_t)yh * W + xh];
              }
            }
          }
          if (!backward) {
            out[o] = sum / count;
            mapping[o] = c_in;
          }
        }
  }
}

/* ---- cpu/ps_roi_pool_kernel.cpp:22-90 (forward: clip to H-1/W-1, round) and :92-155
 * (backward: clip to H/W, roundf) */
void FN(oracle_ps_roi_pool)(const REAL* data, const REAL* rois, REAL* out, int32_t* mapping, int K, int C, int H,
                            int W, int PH, int PW, double spatial_scale, int backward) {
  const REAL scale = (REAL)spatial_scale;
  const int C_out = C / (PH * PW);
  for (int n = 0; n < K; ++n) {
    const REAL* r = rois + 5 * n;
    const int b = (int)r[0];
    int rsw, rsh, rew, reh;
    if (backward) {
      rsw = (int)roundf((float)(r[1] * scale));
      rsh = (int)roundf((float)(r[2] * scale));
      rew = (int)roundf((float)(r[3] * scale));
      reh = (int)roundf((float)(r[4] * scale));
    } else {
      rsw = (int)round(r[1] * scale);
      rsh = (int)round(r[2] * scale);
      rew = (int)round(r[3] * scale);
      reh = (int)round(r[4] * scale);
    }
    const int rw = (rew - rsw) > 1 ? (rew - rsw) : 1, rh = (reh - rsh) > 1 ? (reh - rsh) : 1;
    const REAL bin_h = (REAL)rh / (REAL)PH, bin_w = (REAL)rw / (REAL)PW;
    const int hmax = backward ? H : H - 1, wmax = backward ? W : W - 1;
    for (int co = 0; co < C_out; ++co)
      for (int ph = 0; ph < PH; ++ph)
        for (int pw = 0; pw < PW; ++pw) {
          int hs = (int)floor((REAL)ph * bin_h), ws = (int)floor((REAL)pw * bin_w);
          int he = (int)ceil((REAL)(ph + 1) * bin_h), we = (int)ceil((REAL)(pw + 1) * bin_w);
          hs = hs + rsh < 0 ? 0 : (hs + rsh > hmax ? hmax : hs + rsh);
          he = he + rsh < 0 ? 0 : (he + rsh > hmax ? hmax : he + rsh);
          ws = ws + rsw < 0 ? 0 : (ws + rsw > wmax ? wmax : ws + rsw);
          we = we + rsw < 0 ? 0 : (we + rsw > wmax ? wmax : we + rsw);
          const int empty = (he <= hs) || (we <= ws);
          const size_t o = (((size_t)n * C_out + co) * PH + ph) * PW + pw;
          const int c_in = backward ? mapping[o] : (co * PH + ph) * PW + pw;
          const size_t plane = ((size_t)b * C + c_in) * H * W;
          const REAL bin_area = (REAL)((he - hs) * (we - ws));
          if (backward) {
            const REAL diff = empty ? (REAL)0 : data[o] / bin_area;
            for (int h = hs; h < he; ++h)
              for (int w = ws; w < we; ++w) out[plane + (size_t)h * W + w] += diff;
          } else {
            REAL sum = 0;
            for (int h = hs; h < he; ++h)
              for (int w = ws; w < we; ++w) sum += data[plane + (size_t)h * W + w];
            out[o] = empty ? (REAL)0 : sum / bin_area;
            mapping[o] = c_in;
          }
        }
  }
}

/* ---- cpu/deform_conv2d_kernel.cpp:95-132 */
static REAL FN(dcn_bilinear)(const REAL* in, int H, int W, REAL h, REAL w) {
  if (h <= -1 || H <= h || w <= -1 || W <= w) return 0;
  const int hl = (int)floor(h), wl = (int)floor(w);
  const int hh_ = hl + 1, wh_ = wl + 1;
  const REAL lh = h - hl, lw = w - wl;
  const REAL hh = 1 - lh, hw = 1 - lw;
  REAL v1 = 0, v2 = 0, v3 = 0, v4 = 0;
  if (hl >= 0 && wl >= 0) v1 = in[hl * W + wl];
  if (hl >= 0 && wh_ <= W - 1) v2 = in[hl * W + wh_];
  if (hh_ <= H - 1 && wl >= 0) v3 = in[hh_ * W + wl];
  if (hh_ <= H - 1 && wh_ <= W - 1) v4 = in[hh_ * W + wh_];
  const REAL w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;
  return w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4;
}

/* ---- forward = deformable_im2col (:134-209) contracted with the weights per group
 * (:921-1151): out[b,oc,y,x] = bias[oc] + sum_{ic,i,j} W[oc,ic,i,j] * mask * bilinear(...).
 * The contraction is accumulated in double and rounded once (the reference uses a BLAS GEMM
 * whose summation order is unspecified; parity is judged at 1e-4).
 * The columns of one output row of a group are sampled once and shared by the group's OC / groups
 * output channels; every output still sums its (ic, i, j) terms in that order. */
void FN(oracle_deform_conv2d)(const REAL* in, const REAL* weight, const REAL* offset, const REAL* mask,
                              const REAL* bias, REAL* out, int B, int C, int H, int W, int OC, int kh, int kw, int sh,
                              int sw, int ph, int pw, int dh, int dw, int groups, int ogroups, int use_mask) {
  const int oh = (H + 2 * ph - (dh * (kh - 1) + 1)) / sh + 1;
  const int ow = (W + 2 * pw - (dw * (kw - 1) + 1)) / sw + 1;
  const int ICg = C / groups, OCg = OC / groups, cpog = C / ogroups, KK = kh * kw;
  const size_t plane = (size_t)oh * ow;
  REAL* cols = (REAL*)malloc(sizeof(REAL) * (size_t)ICg * KK * (ow > 0 ? ow : 1));   /* [ICg * KK][ow] */
  double* acc = (double*)malloc(sizeof(double) * (size_t)(ow > 0 ? ow : 1));
  for (int b = 0; b < B; ++b)
    for (int g = 0; g < groups; ++g)
      for (int y = 0; y < oh; ++y) {
        for (int ic = 0; ic < ICg; ++ic) {
          const int c = g * ICg + ic, og = c / cpog;
          const REAL* ip = in + ((size_t)b * C + c) * H * W;
          const REAL* op = offset + ((size_t)(b * ogroups + og) * 2 * KK) * plane;
          const REAL* mp = mask + ((size_t)(b * ogroups + og) * KK) * plane;
          for (int i = 0; i < kh; ++i)
            for (int j = 0; j < kw; ++j) {
              const int t = i * kw + j;
              REAL* cp = cols + ((size_t)ic * KK + t) * ow;
              for (int x = 0; x < ow; ++x) {
                const REAL mval = use_mask ? mp[(size_t)t * plane + (size_t)y * ow + x] : (REAL)1;
                const REAL off_h = op[(size_t)(2 * t) * plane + (size_t)y * ow + x];
                const REAL off_w = op[(size_t)(2 * t + 1) * plane + (size_t)y * ow + x];
                const REAL yy = (y * sh - ph) + i * dh + off_h;
                const REAL xx = (x * sw - pw) + j * dw + off_w;
                cp[x] = mval * FN(dcn_bilinear)(ip, H, W, yy, xx);
              }
            }
        }
        for (int oc = g * OCg; oc < (g + 1) * OCg; ++oc) {
          const REAL* wp = weight + (size_t)oc * ICg * KK;
          for (int x = 0; x < ow; ++x) acc[x] = 0;
          for (size_t k = 0; k < (size_t)ICg * KK; ++k) {
            const double wv = (double)wp[k];
            const REAL* cp = cols + k * ow;
            for (int x = 0; x < ow; ++x) acc[x] += wv * (double)cp[x];
          }
          REAL* orow = out + (((size_t)b * OC + oc) * oh + y) * ow;
          for (int x = 0; x < ow; ++x) orow[x] = (REAL)(acc[x] + (double)bias[oc]);
        }
      }
  free(cols);
  free(acc);
}

/* ---- box_iou_rotated_utils.h:67-383 via cpu/box_iou_rotated_kernel.cpp:29-115 */
typedef struct {
  REAL x, y;
} FN(pt);

static REAL FN(cross2)(FN(pt) a, FN(pt) b) { return a.x * b.y - b.x * a.y; }
static REAL FN(dot2)(FN(pt) a, FN(pt) b) { return a.x * b.x + a.y * b.y; }
static FN(pt) FN(psub)(FN(pt) a, FN(pt) b) {
  FN(pt) r = {a.x - b.x, a.y - b.y};
  return r;
}

static void FN(rot_corners)(REAL cx, REAL cy, REAL w, REAL h, REAL a, FN(pt) * p) {
  const double theta = a * 0.01745329251;
  const REAL c2 = (REAL)cos(theta) * 0.5f, s2 = (REAL)sin(theta) * 0.5f;
  p[0].x = cx + s2 * h + c2 * w;
  p[0].y = cy + c2 * h - s2 * w;
  p[1].x = cx - s2 * h + c2 * w;
  p[1].y = cy - c2 * h - s2 * w;
  p[2].x = 2 * cx - p[0].x;
  p[2].y = 2 * cy - p[0].y;
  p[3].x = 2 * cx - p[1].x;
  p[3].y = 2 * cy - p[1].y;
}

static REAL FN(rot_iou)(const REAL* r1, const REAL* r2) {
  const double sx = (r1[0] + r2[0]) / 2.0, sy = (r1[1] + r2[1]) / 2.0;
  const REAL x1 = (REAL)(r1[0] - sx), y1 = (REAL)(r1[1] - sy), x2 = (REAL)(r2[0] - sx), y2 = (REAL)(r2[1] - sy);
  const REAL area1 = r1[2] * r1[3], area2 = r2[2] * r2[3];
  if (area1 < 1e-14 || area2 < 1e-14) return 0.f;
  FN(pt) a[4], b[4], ea[4], eb[4], cand[24], q[24];
  FN(rot_corners)(x1, y1, r1[2], r1[3], r1[4], a);
  FN(rot_corners)(x2, y2, r2[2], r2[3], r2[4], b);
  for (int i = 0; i < 4; ++i) {
    ea[i] = FN(psub)(a[(i + 1) % 4], a[i]);
    eb[i] = FN(psub)(b[(i + 1) % 4], b[i]);
  }
  const double EPS = 1e-5;
  int num = 0;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      const REAL det = FN(cross2)(eb[j], ea[i]);
      if (fabs(det) <= 1e-14) continue;
      const FN(pt) d = FN(psub)(b[j], a[i]);
      const REAL t1 = FN(cross2)(eb[j], d) / det, t2 = FN(cross2)(ea[i], d) / det;
      if (t1 > -EPS && t1 < 1.0f + EPS && t2 > -EPS && t2 < 1.0f + EPS) {
        cand[num].x = a[i].x + ea[i].x * t1;
        cand[num].y = a[i].y + ea[i].y * t1;
        ++num;
      }
    }
  for (int pass = 0; pass < 2; ++pass) {
    const FN(pt)* pq = pass ? b : a;
    const FN(pt)* pr = pass ? a : b;
    const FN(pt) AB = pass ? ea[0] : eb[0], DA = pass ? ea[3] : eb[3];
    const REAL ABAB = FN(dot2)(AB, AB), ADAD = FN(dot2)(DA, DA);
    for (int i = 0; i < 4; ++i) {
      const FN(pt) AP = FN(psub)(pq[i], pr[0]);
      const REAL pAB = FN(dot2)(AP, AB), pAD = -FN(dot2)(AP, DA);
      if ((pAB > -EPS) && (pAD > -EPS) && (pAB < ABAB + EPS) && (pAD < ADAD + EPS)) cand[num++] = pq[i];
    }
  }
  REAL inter = 0;
  if (num > 2) {
    /* convex_hull_graham, CPU branch (:173-305) */
    int t = 0;
    for (int i = 1; i < num; ++i)
      if (cand[i].y < cand[t].y || (cand[i].y == cand[t].y && cand[i].x < cand[t].x)) t = i;
    const FN(pt) start = cand[t];
    for (int i = 0; i < num; ++i) q[i] = FN(psub)(cand[i], start);
    FN(pt) tmp = q[0];
    q[0] = q[t];
    q[t] = tmp;
    REAL dist[24];
    for (int i = 0; i < num; ++i) dist[i] = FN(dot2)(q[i], q[i]);
    for (int i = 1; i < num - 1; ++i)
      for (int j = i + 1; j < num; ++j) {
        const REAL cp = FN(cross2)(q[i], q[j]);
        if ((cp < -1e-6) || (fabs(cp) < 1e-6 && dist[i] > dist[j])) {
          FN(pt) tq = q[i];
          q[i] = q[j];
          q[j] = tq;
          REAL td = dist[i];
          dist[i] = dist[j];
          dist[j] = td;
        }
      }
    for (int i = 0; i < num; ++i) dist[i] = FN(dot2)(q[i], q[i]);
    int k = 1, m = 1;
    for (; k < num; ++k)
      if (dist[k] > 1e-8) break;
    if (k < num) {
      q[1] = q[k];
      m = 2;
      for (int i = k + 1; i < num; ++i) {
        while (m > 1) {
          const FN(pt) q1 = FN(psub)(q[i], q[m - 2]), q2 = FN(psub)(q[m - 1], q[m - 2]);
          if (q1.x * q2.y >= q2.x * q1.y)
            --m;
          else
            break;
        }
        q[m++] = q[i];
      }
    }
    if (m > 2) {
      REAL area = 0;
      for (int i = 1; i < m - 1; ++i) area += (REAL)fabs(FN(cross2)(FN(psub)(q[i], q[0]), FN(psub)(q[i + 1], q[0])));
      inter = (REAL)(area / 2.0);
    }
  }
  REAL iou = inter / (area1 + area2 - inter);
  iou = (iou < 0) ? 0 : (iou > 1 ? 1 : iou);
  return iou;
}

void FN(oracle_box_iou_rotated)(const REAL* b1, const REAL* b2, float* out, int N, int M) {
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < M; ++j) out[(size_t)i * M + j] = (float)FN(rot_iou)(b1 + 5 * i, b2 + 5 * j);
}

/* A sampling coordinate of the backward, `(out_y * stride_h - pad_h) + i * dilation_h + offset_h` (:301-302, :525-526).
 * coord_f32: round it to float as the reference's fp32 build does (scalar_t = float), for a double evaluation of an fp32
 * problem — the coordinate weight jumps where the coordinate crosses an integer, so the rounding decides which rows it sees. */
static REAL FN(dcn_coord)(int base, REAL off, int coord_f32) {
  const REAL v = base + off;
  return coord_f32 ? (REAL)(float)v : v;
}

/* ---- deformable_im2col (cpu/deform_conv2d_kernel.cpp:134-209) for image b: cols[(c * kh + i) * kw + j][y * ow + x] =
 * mask * bilinear(...), the `columns` that backward_gradient_parameters (:1050-1151) contracts with grad_out. */
void FN(oracle_deform_conv2d_im2col)(const REAL* in, const REAL* offset, const REAL* mask, REAL* cols, int b, int C, int H,
                                     int W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int ogroups,
                                     int use_mask, int coord_f32) {
  const int oh = (H + 2 * ph - (dh * (kh - 1) + 1)) / sh + 1;
  const int ow = (W + 2 * pw - (dw * (kw - 1) + 1)) / sw + 1;
  const int KK = kh * kw, cpog = C / ogroups;
  const size_t plane = (size_t)oh * ow;
  for (int c = 0; c < C; ++c) {
    const int og = c / cpog;
    const REAL* ip = in + ((size_t)b * C + c) * H * W;
    const REAL* op = offset + ((size_t)(b * ogroups + og) * 2 * KK) * plane;
    const REAL* mp = mask + ((size_t)(b * ogroups + og) * KK) * plane;
    for (int i = 0; i < kh; ++i)
      for (int j = 0; j < kw; ++j) {
        const int t = i * kw + j;
        REAL* cp = cols + ((size_t)c * KK + t) * plane;
        for (int y = 0; y < oh; ++y)
          for (int x = 0; x < ow; ++x) {
            const size_t pix = (size_t)y * ow + x;
            const REAL mval = use_mask ? mp[(size_t)t * plane + pix] : (REAL)1;
            const REAL yy = FN(dcn_coord)((y * sh - ph) + i * dh, op[(size_t)(2 * t) * plane + pix], coord_f32);
            const REAL xx = FN(dcn_coord)((x * sw - pw) + j * dw, op[(size_t)(2 * t + 1) * plane + pix], coord_f32);
            cp[pix] = mval * FN(dcn_bilinear)(ip, H, W, yy, xx);
          }
      }
  }
}

/* ---- cpu/deform_conv2d_kernel.cpp:407-438 (get_coordinate_weight): the corner validity alone, NOT gated by the
 * location test of bilinear_interpolate (a sample at y == -1 exactly still sees row 0). */
static REAL FN(dcn_coordinate_weight)(const REAL* im, int H, int W, REAL y, REAL x, int is_y_direction) {
  const int yl = (int)floor(y), xl = (int)floor(x);
  const int yh = yl + 1, xh = xl + 1;
  const int vyl = 0 <= yl && yl < H, vyh = 0 <= yh && yh < H;
  const int vxl = 0 <= xl && xl < W, vxh = 0 <= xh && xh < W;
  const REAL v_yx = (vyl && vxl) ? im[yl * W + xl] : (REAL)0;
  const REAL v_yX = (vyl && vxh) ? im[yl * W + xh] : (REAL)0;
  const REAL v_Yx = (vyh && vxl) ? im[yh * W + xl] : (REAL)0;
  const REAL v_YX = (vyh && vxh) ? im[yh * W + xh] : (REAL)0;
  if (is_y_direction) {
    const REAL dx = x - xl;
    return dx * (v_YX - v_yX) + (1 - dx) * (v_Yx - v_yx);
  }
  const REAL dy = y - yl;
  return dy * (v_YX - v_Yx) + (1 - dy) * (v_yX - v_yx);
}

/* ---- the data gradients of image b from its `columns` (cols[(c * kh + i) * kw + j][y * ow + x] = W^T x grad_out per
 * weight group, formed by the caller as backward_gradient_inputs does, :1000-1048):
 *   grad_input  += deformable_col2im (:274-348): mask * (1 - |y - yp|) * (1 - |x - xp|) * column, for the corners
 *                  yp in int(y) + {-1, 0, 1} with |y - yp| < 1 (the same gate as bilinear_interpolate);
 *   grad_offset  = deformable_col2im_coord (:440-551): sum over the offset group's channels of mask * coordinate weight
 *                  * column, component 2t = y, 2t + 1 = x;
 *   grad_mask    = sum of column * bilinear(...) over the same channels (only with use_mask; the caller zeroes it).
 * grad_input must be zeroed by the caller; grad_offset / grad_mask rows of image b are overwritten. */
void FN(oracle_deform_conv2d_backward)(const REAL* cols, const REAL* in, const REAL* offset, const REAL* mask,
                                       REAL* grad_in, REAL* grad_off, REAL* grad_mask, int b, int C, int H, int W, int kh,
                                       int kw, int sh, int sw, int ph, int pw, int dh, int dw, int ogroups, int use_mask,
                                       int coord_f32) {
  const int oh = (H + 2 * ph - (dh * (kh - 1) + 1)) / sh + 1;
  const int ow = (W + 2 * pw - (dw * (kw - 1) + 1)) / sw + 1;
  const int KK = kh * kw, cpog = C / ogroups;
  const size_t plane = (size_t)oh * ow;
  /* col2im */
  for (int c = 0; c < C; ++c) {
    const int og = c / cpog;
    const REAL* op = offset + ((size_t)(b * ogroups + og) * 2 * KK) * plane;
    const REAL* mp = mask + ((size_t)(b * ogroups + og) * KK) * plane;
    REAL* gp = grad_in + ((size_t)b * C + c) * H * W;
    for (int i = 0; i < kh; ++i)
      for (int j = 0; j < kw; ++j) {
        const int t = i * kw + j;
        const REAL* cp = cols + ((size_t)c * KK + t) * plane;
        for (int oy = 0; oy < oh; ++oy)
          for (int ox = 0; ox < ow; ++ox) {
            const size_t pix = (size_t)oy * ow + ox;
            const REAL mval = use_mask ? mp[(size_t)t * plane + pix] : (REAL)1;
            const REAL y = FN(dcn_coord)((oy * sh - ph) + i * dh, op[(size_t)(2 * t) * plane + pix], coord_f32);
            const REAL x = FN(dcn_coord)((ox * sw - pw) + j * dw, op[(size_t)(2 * t + 1) * plane + pix], coord_f32);
            for (int ddy = -1; ddy <= 1; ++ddy)
              for (int ddx = -1; ddx <= 1; ++ddx) {
                const int yp = (int)y + ddy, xp = (int)x + ddx;
                if (0 <= yp && yp < H && 0 <= xp && xp < W && fabs(y - yp) < 1 && fabs(x - xp) < 1) {
                  const REAL wgt = (1 - (REAL)fabs(y - yp)) * (1 - (REAL)fabs(x - xp));
                  gp[(size_t)yp * W + xp] += mval * wgt * cp[pix];
                }
              }
          }
      }
  }
  /* col2im_coord */
  for (int og = 0; og < ogroups; ++og) {
    const REAL* op = offset + ((size_t)(b * ogroups + og) * 2 * KK) * plane;
    const REAL* mp = mask + ((size_t)(b * ogroups + og) * KK) * plane;
    REAL* gop = grad_off + ((size_t)(b * ogroups + og) * 2 * KK) * plane;
    REAL* gmp = grad_mask + ((size_t)(b * ogroups + og) * KK) * plane;
    for (int oc = 0; oc < 2 * KK; ++oc) {
      const int t = oc / 2, i = t / kw, j = t % kw, is_y = oc % 2 == 0;
      for (int oy = 0; oy < oh; ++oy)
        for (int ox = 0; ox < ow; ++ox) {
          const size_t pix = (size_t)oy * ow + ox;
          const REAL mval = use_mask ? mp[(size_t)t * plane + pix] : (REAL)1;
          const REAL y = FN(dcn_coord)((oy * sh - ph) + i * dh, op[(size_t)(2 * t) * plane + pix], coord_f32);
          const REAL x = FN(dcn_coord)((ox * sw - pw) + j * dw, op[(size_t)(2 * t + 1) * plane + pix], coord_f32);
          REAL goff = 0, gm = 0;
          for (int c = og * cpog; c < (og + 1) * cpog; ++c) {
            const REAL* im = in + ((size_t)b * C + c) * H * W;
            const REAL col = cols[((size_t)c * KK + t) * plane + pix];
            goff += mval * FN(dcn_coordinate_weight)(im, H, W, y, x, is_y) * col;
            if (use_mask && is_y) gm += col * FN(dcn_bilinear)(im, H, W, y, x);
          }
          gop[(size_t)oc * plane + pix] = goff;
          if (use_mask && is_y) gmp[(size_t)t * plane + pix] = gm;
        }
    }
  }
}
