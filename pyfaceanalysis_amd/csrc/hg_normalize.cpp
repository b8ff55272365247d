// Pose-normalised face crops on the host (include/higsfa.h, "normalize_image"): the geometry of face_normalization_tools.normalize_image
// for the configuration both reference callers use, and PIL's pixels — crop (a shift), crop.rotate(angle, BICUBIC), the EXTENT / BICUBIC cut —
// restated from Geometry.c.  Plain C++ without HIP, compiled with contraction off: every double operation below rounds on its own, as
// Python floats and PIL's C doubles do, and atan2 / cos / sin / sqrt / pow are the host libm's — the library Python's math calls on the
// machine this runs on.  The device path (hg_normalize.hip) takes the geometry from here and repeats the pixel arithmetic.
#include "hg_normalize.hpp"

#include "hg_frame_list.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace hg {

namespace {

constexpr double kPi = 3.14159265358979323846;      // math.pi

// Python's round(v, 15) for |v| <= 1: the decimal nearest to v's exact value, ties to even, then the double nearest to that decimal.
// v = mant 2^e exactly, and mant 10^15 < 2^103 fits 128 bits: the quotient and the remainder of the shift decide without any rounding.
double round15(double v) {
    if (!(std::fabs(v) <= 1.0) || v == 0.0) return v;
    int ex = 0;
    const double fr = std::frexp(std::fabs(v), &ex);                    // |v| = fr 2^ex, 0.5 <= fr < 1
    const unsigned __int128 N = (unsigned __int128)(uint64_t)std::ldexp(fr, 53) * 1000000000000000ull;
    const int sh = 53 - ex;                                             // |v| 10^15 = N / 2^sh, sh >= 52
    unsigned __int128 k = 0;
    if (sh < 128) {
        k = N >> sh;
        const unsigned __int128 rem = N & (((unsigned __int128)1 << sh) - 1), half = (unsigned __int128)1 << (sh - 1);
        if (rem > half || (rem == half && (k & 1))) ++k;
    }
    return std::copysign((double)(uint64_t)k / 1e15, v);
}

double py_mod(double v, double w) {      // Python's float %: the result carries the divisor's sign
    double m = std::fmod(v, w);
    if (m != 0.0) {
        if ((w < 0.0) != (m < 0.0)) m += w;
    } else {
        m = std::copysign(0.0, w);
    }
    return m;
}

// ---- PIL's affine_transform + bicubic_filter8 (Geometry.c), as in hg_filter_dev.hpp -------------------------------------------------
constexpr int32_t kOutside = INT32_MIN;
struct Ent {
    double d;
    int32_t i;
};

inline Ent coord(double s, int lim) {
    if (!(s >= 0.0 && s < (double)lim)) return Ent{0.0, kOutside};      // (NaN is outside)
    s = s - 0.5;
    const int32_t i = s < 0.0 ? (int32_t)std::floor(s) : (int32_t)s;
    return Ent{s - (double)i, i};
}

inline double bicubic(double v1, double v2, double v3, double v4, double d) {
    const double p1 = v2;
    const double p2 = -v1 + v3;
    const double p3 = 2.0 * (v1 - v2) + v3 - v4;
    const double p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}

inline int clip(int v, int lim) { return v < 0 ? 0 : v < lim ? v : lim - 1; }

template <typename Tap>
inline uint8_t sample(Tap&& tap, int x, double dx, int y, double dy, int W, int H) {
    const int x0 = clip(x - 1, W), x1 = clip(x, W), x2 = clip(x + 1, W), x3 = clip(x + 2, W);
    auto row = [&](int yy) { return bicubic(tap(x0, yy), tap(x1, yy), tap(x2, yy), tap(x3, yy), dx); };
    const double r1 = row(y - 1 < 0 ? 0 : y - 1);
    const double r2 = y >= 0 ? row(y) : r1;
    const double r3 = y + 1 < H ? row(y + 1) : r2;
    const double r4 = y + 2 < H ? row(y + 2) : r3;
    const double v = bicubic(r1, r2, r3, r4, dy);
    return v <= 0.0 ? (uint8_t)0 : v >= 255.0 ? (uint8_t)255 : (uint8_t)(int)v;
}

// the source coordinate of output index i of an EXTENT axis (lo, hi) cut into n pixels: a (i + 0.5) + lo with a = (hi - lo) / n
inline Ent extent_entry(double lo, double hi, int n, int i, int lim) {
    const double a = (hi - lo) / (double)n;
    return coord(a * ((double)i + 0.5) + lo, lim);
}

// the columns (rows) of a lim-wide image the cut of one axis reads: x - 1 .. x + 2 of every inside entry, clipped
void axis_range(double lo, double hi, int n, int lim, int32_t& first, int32_t& count) {
    int a = INT32_MAX, b = INT32_MIN;
    for (int i = 0; i < n; ++i) {
        const Ent e = extent_entry(lo, hi, n, i, lim);
        if (e.i == kOutside) continue;
        a = std::min(a, clip(e.i - 1, lim));
        b = std::max(b, clip(e.i + 2, lim));
    }
    first = b >= a ? a : 0;
    count = b >= a ? b - a + 1 : 0;
}

struct Frame {
    const uint8_t* p;
    int h, w;
    int64_t ld;
};

// pixel (xc, yc) of the virtual crop: the frame shifted by the crop origin, 0 outside the frame
inline double crop_px(const Frame& f, const hg_norm_geom& g, int xc, int yc) {
    const int64_t fx = (int64_t)xc + g.crop_x0, fy = (int64_t)yc + g.crop_y0;
    return (fx >= 0 && fx < f.w && fy >= 0 && fy < f.h) ? (double)f.p[fy * f.ld + fx] : 0.0;
}

// pixel (xr, yr) of crop.rotate(angle, BICUBIC)
inline uint8_t rot_px(const Frame& f, const hg_norm_geom& g, int xr, int yr) {
    if (!g.rotated) return (uint8_t)crop_px(f, g, xr, yr);
    const double xin = (double)xr + 0.5, yin = (double)yr + 0.5;
    const Ent ex = coord(g.m[0] * xin + g.m[1] * yin + g.m[2], g.W);
    const Ent ey = coord(g.m[3] * xin + g.m[4] * yin + g.m[5], g.H);
    if (ex.i == kOutside || ey.i == kOutside) return 0;
    return sample([&](int xc, int yc) { return crop_px(f, g, xc, yc); }, ex.i, ex.d, ey.i, ey.d, g.W, g.H);
}

const char* geom_check(const hg_norm_geom& g, int frame_w, int frame_h) {
    if (g.status < 0 || g.status > HG_NORM_CENTRE_RANGE) return "normalize: a geom with an unknown status";
    if (g.status != 0) return nullptr;
    if (g.W < 1 || g.H < 1 || !(g.W & 1) || !(g.H & 1)) return "normalize: a geom whose crop size is not positive and odd";
    const int64_t cxi = (int64_t)g.crop_x0 + (g.W - 1) / 2, cyi = (int64_t)g.crop_y0 + (g.H - 1) / 2;
    if ((int64_t)g.W != 2 * std::max<int64_t>((int64_t)frame_w - 1 - cxi, cxi) + 1 || (int64_t)g.H != 2 * std::max<int64_t>((int64_t)frame_h - 1 - cyi, cyi) + 1)
        return "normalize: a geom built for another frame size";
    const int32_t* r = g.rect;
    if (r[2] < 0 || r[3] < 0 || ((r[2] == 0) != (r[3] == 0))) return "normalize: a geom with a malformed rect";
    if (r[2] > 0 && (r[0] < 0 || r[1] < 0 || (int64_t)r[0] + r[2] > g.W || (int64_t)r[1] + r[3] > g.H)) return "normalize: a geom whose rect leaves the crop";
    return nullptr;
}

}  // namespace

const char* normalize_geometry_host(const double* eyes, int64_t n, int frame_w, int frame_h, const hg_norm_consts* consts, hg_norm_geom* out) {
    if (n < 0) return "normalize: n < 0";
    if (!consts) return "normalize: null consts";
    if (n > 0 && (!eyes || !out)) return "normalize: null data pointer";
    if (consts->out_w < 1 || consts->out_h < 1 || consts->out_w > 4096 || consts->out_h > 4096) return "normalize: out_w / out_h must be 1 .. 4096";
    if (consts->method != HG_NORM_AREA && consts->method != HG_NORM_AREAZ) return "normalize: unknown scale method (0 area, 1 areaZ)";
    if (consts->rotate != 0 && consts->rotate != 1) return "normalize: rotate must be 0 or 1";
    if (frame_w < 1 || frame_h < 1 || frame_w > (1 << 24) || frame_h > (1 << 24)) return "normalize: frame_w / frame_h must be 1 .. 2^24";
    volatile double two = 2.0;      // (37.5 / 37.0) ** 2 is libm's pow at run time, as in Python; not a compile-time constant
    const double desired_area = 37.0 * 42.0 / 2.0 * std::pow(37.5 / 37.0, two);
    for (int64_t f = 0; f < n; ++f) {
        hg_norm_geom g;
        std::memset(&g, 0, sizeof g);
        const double lx = eyes[f * 4], ly = eyes[f * 4 + 1], rx = eyes[f * 4 + 2], ry = eyes[f * 4 + 3];
        auto refuse = [&](int status) {
            g.status = status;
            out[f] = g;
        };
        if (!(std::isfinite(lx) && std::isfinite(ly) && std::isfinite(rx) && std::isfinite(ry))) {
            refuse(HG_NORM_NOT_FINITE);
            continue;
        }
        if (lx > rx) {
            refuse(HG_NORM_EYES_SWAPPED);
            continue;
        }
        const double exm = (rx + lx) / 2.0, eym = (ry + ly) / 2.0;
        const double ddx = lx - rx, ddy = ly - ry;
        const double dist = std::sqrt(ddx * ddx + ddy * ddy);
        if (!(dist > 0.0) || !std::isfinite(dist)) {      // (an overflowing distance has no finite geometry either)
            refuse(std::isfinite(dist) ? HG_NORM_ZERO_DISTANCE : HG_NORM_NOT_FINITE);
            continue;
        }
        const double eye_dx = rx - lx, eye_dy = ry - ly;
        const double eye_line_angle = std::atan2(eye_dy, eye_dx) * 180 / kPi;
        const double mx = exm - (42.0 / 37.0) * eye_dy, my = eym + (42.0 / 37.0) * eye_dx;
        const double hx = exm - mx, hy = eym - my;
        const double height = std::sqrt(hx * hx + hy * hy);
        const double area = dist * height / 2.0;
        const double scale = std::sqrt(area / desired_area);
        double ori_w = consts->out_w * scale, ori_h = consts->out_h * scale;
        if (consts->method == HG_NORM_AREAZ) {
            ori_w = ori_w / 2;
            ori_h = ori_h / 2;
        }
        const double cx = (exm + mx) / 2.0, cy = (eym + my) / 2.0;
        if (!(std::fabs(cx) <= 1048576.0 && std::fabs(cy) <= 1048576.0)) {
            refuse(HG_NORM_CENTRE_RANGE);
            continue;
        }
        const int32_t cxi = (int32_t)(cx + 0.5), cyi = (int32_t)(cy + 0.5);      // Python's int(): truncation
        const double win_w = 2 * std::max((double)(frame_w - 1 - cxi) + 0.5, (double)cxi + 0.5);
        const double win_h = 2 * std::max((double)(frame_h - 1 - cyi) + 0.5, (double)cyi + 0.5);
        g.W = (int32_t)(win_w + 0.5);
        g.H = (int32_t)(win_h + 0.5);
        g.crop_x0 = (int32_t)((double)cxi - (win_w - 1) / 2.0);
        g.crop_y0 = (int32_t)((double)cyi - (win_h - 1) / 2.0);
        g.angle = consts->rotate ? eye_line_angle : 0.0;
        const double dx = cx - (double)cxi, dy = cy - (double)cyi;
        const double rad = -g.angle * kPi / 180.0;
        const double c = std::cos(rad), s = std::sin(rad);
        g.shift[0] = dx * c - dy * s;
        g.shift[1] = dy * c + dx * s;
        const double ncx = (double)(g.W - 1) / 2.0 + g.shift[0], ncy = (double)(g.H - 1) / 2.0 + g.shift[1];
        g.box[0] = ncx - (ori_w - 1) / 2.0;
        g.box[1] = ncy - (ori_h - 1) / 2.0;
        g.box[2] = (ncx + (ori_w - 1) / 2.0) + 1;
        g.box[3] = (ncy + (ori_h - 1) / 2.0) + 1;
        // Image.rotate(angle) on a W x H image, default centre
        const double a = py_mod(g.angle, 360.0);
        g.rotated = a != 0.0 ? 1 : 0;
        if (g.rotated) {
            const double r = -(a * (kPi / 180.0));      // -math.radians(angle)
            g.m[0] = round15(std::cos(r));
            g.m[1] = round15(std::sin(r));
            g.m[3] = round15(-std::sin(r));
            g.m[4] = round15(std::cos(r));
            const double ccx = (double)g.W / 2.0, ccy = (double)g.H / 2.0;
            const double x = -ccx, y = -ccy;
            g.m[2] = g.m[0] * x + g.m[1] * y + 0.0;
            g.m[5] = g.m[3] * x + g.m[4] * y + 0.0;
            g.m[2] += ccx;
            g.m[5] += ccy;
        } else {
            g.m[0] = g.m[4] = 1.0;
        }
        axis_range(g.box[0], g.box[2], consts->out_w, g.W, g.rect[0], g.rect[2]);
        axis_range(g.box[1], g.box[3], consts->out_h, g.H, g.rect[1], g.rect[3]);
        if (g.rect[2] == 0 || g.rect[3] == 0) g.rect[0] = g.rect[1] = g.rect[2] = g.rect[3] = 0;
        out[f] = g;
    }
    return nullptr;
}

const char* normalize_check(const void* frame, int frame_h, int frame_w, int64_t ld, const hg_norm_geom* geoms, int64_t n, int out_w, int out_h,
                            const void* out, int64_t ldo) {
    if (n < 0) return "normalize: n < 0";
    if (frame_h <= 0 || frame_w <= 0 || frame_w > (1 << 24) || frame_h > (1 << 24)) return "normalize: bad frame size";
    if (ld < frame_w) return "normalize: ld < frame_w";
    if (out_w < 1 || out_h < 1 || out_w > 4096 || out_h > 4096) return "normalize: out_w / out_h must be 1 .. 4096";
    if (ldo < (int64_t)out_w * out_h) return "normalize: ldo < out_w * out_h";
    if (n > 0 && (!frame || !geoms || !out)) return "normalize: null data pointer";
    for (int64_t f = 0; f < n; ++f)
        if (const char* why = geom_check(geoms[f], frame_w, frame_h)) return why;
    return nullptr;
}

namespace {

// the shape of a stack: n, the frame size and ld as normalize_check reads them, then the stack's own two numbers
const char* stack_shape_check(int n_frames, int64_t frame_stride, int frame_h, int frame_w, int64_t ld, int64_t n) {
    if (n < 0) return "normalize: n < 0";
    if (frame_h <= 0 || frame_w <= 0 || frame_w > (1 << 24) || frame_h > (1 << 24)) return "normalize: bad frame size";
    if (ld < frame_w) return "normalize: ld < frame_w";
    if (n_frames < 1 || n_frames > HG_MAX_STACK_FRAMES) return "normalize: n_frames must be 1 .. HG_MAX_STACK_FRAMES";
    // frame_stride >= (frame_h - 1) ld + frame_w, without forming the product (ld is any int64)
    if (frame_stride < frame_w || (frame_h > 1 && (frame_stride - frame_w) / (frame_h - 1) < ld)) return "normalize: frame_stride < (frame_h - 1) ld + frame_w";
    return nullptr;
}

const char* geoms_check(const hg_norm_geom* geoms, int64_t n, int frame_w, int frame_h) {
    for (int64_t f = 0; f < n; ++f)
        if (const char* why = geom_check(geoms[f], frame_w, frame_h)) return why;
    return nullptr;
}

}  // namespace

const char* normalize_stack_check(const void* frames, int n_frames, int64_t frame_stride, int frame_h, int frame_w, int64_t ld, const hg_norm_geom* geoms,
                                  const int32_t* face_frame, int64_t n) {
    if (const char* why = stack_shape_check(n_frames, frame_stride, frame_h, frame_w, ld, n)) return why;
    if (n > 0 && (!frames || !geoms || !face_frame)) return "normalize: null data pointer";
    return geoms_check(geoms, n, frame_w, frame_h);
}

const char* normalize_frames_check(const void* frames, int n_frames, int64_t frame_stride, int frame_h, int frame_w, int64_t ld, const hg_norm_geom* geoms,
                                   const int32_t* face_frame, int64_t n, int out_w, int out_h, const void* out, int64_t ldo) {
    if (const char* why = stack_shape_check(n_frames, frame_stride, frame_h, frame_w, ld, n)) return why;
    if (out_w < 1 || out_h < 1 || out_w > 4096 || out_h > 4096) return "normalize: out_w / out_h must be 1 .. 4096";
    if (ldo < (int64_t)out_w * out_h) return "normalize: ldo < out_w * out_h";
    if (n > 0 && (!frames || !geoms || !face_frame || !out)) return "normalize: null data pointer";
    return geoms_check(geoms, n, frame_w, frame_h);
}

namespace {

// the list itself: n, the number of frames, every descriptor
std::string list_shape_check(const hg_frame_ref* frames, int n_frames, int64_t n) {
    if (n < 0) return "normalize: n < 0";
    if (n_frames < 1 || n_frames > HG_MAX_STACK_FRAMES) return "normalize: n_frames must be 1 .. HG_MAX_STACK_FRAMES";
    if (!frames) return "normalize: null frame list";
    for (int f = 0; f < n_frames; ++f) {
        const hg_frame_ref& F = frames[f];
        std::string bad = list_frame_refusal(f, F.frame_dev, F.frame_h, F.frame_w, F.ld, 1);
        if (!bad.empty()) return bad;
        if (F.frame_w > (1 << 24) || F.frame_h > (1 << 24)) return "frame " + std::to_string(f) + " of the list: larger than 2^24 pixels per side";
    }
    return "";
}

// every face's geom against its own frame's size
std::string list_geoms_check(const hg_frame_ref* frames, int n_frames, const hg_norm_geom* geoms, const int32_t* face_frame, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        const int32_t f = face_frame[i];
        if (f < 0 || f >= n_frames) continue;
        if (const char* why = geom_check(geoms[i], frames[f].frame_w, frames[f].frame_h))
            return std::string(why) + " (face " + std::to_string((long long)i) + ", on frame " + std::to_string(f) + " of the list)";
    }
    return "";
}

}  // namespace

std::string normalize_list_check(const hg_frame_ref* frames, int n_frames, const hg_norm_geom* geoms, const int32_t* face_frame, int64_t n) {
    std::string why = list_shape_check(frames, n_frames, n);
    if (!why.empty()) return why;
    if (n > 0 && (!geoms || !face_frame)) return "normalize: null data pointer";
    return list_geoms_check(frames, n_frames, geoms, face_frame, n);
}

std::string normalize_frame_list_check(const hg_frame_ref* frames, int n_frames, const hg_norm_geom* geoms, const int32_t* face_frame, int64_t n, int out_w,
                                       int out_h, const void* out, int64_t ldo) {
    std::string why = list_shape_check(frames, n_frames, n);
    if (!why.empty()) return why;
    if (out_w < 1 || out_h < 1 || out_w > 4096 || out_h > 4096) return "normalize: out_w / out_h must be 1 .. 4096";
    if (ldo < (int64_t)out_w * out_h) return "normalize: ldo < out_w * out_h";
    if (n > 0 && (!geoms || !face_frame || !out)) return "normalize: null data pointer";
    return list_geoms_check(frames, n_frames, geoms, face_frame, n);
}

const char* normalize_faces_host(const uint8_t* frame, int frame_h, int frame_w, int64_t ld, const hg_norm_geom* geoms, int64_t n, int out_w, int out_h,
                                 uint8_t* out, int64_t ldo) {
    if (const char* why = normalize_check(frame, frame_h, frame_w, ld, geoms, n, out_w, out_h, out, ldo)) return why;
    const Frame fr{frame, frame_h, frame_w, ld};
    std::vector<uint8_t> rot;
    for (int64_t f = 0; f < n; ++f) {
        const hg_norm_geom& g = geoms[f];
        uint8_t* dst = out + f * ldo;
        if (g.status != 0 || g.rect[2] == 0) {
            std::memset(dst, 0, (size_t)out_w * out_h);
            continue;
        }
        const int rx0 = g.rect[0], ry0 = g.rect[1], rw = g.rect[2], rh = g.rect[3];
        const bool staged = (int64_t)rw * rh <= normalize_stage_limit(out_w, out_h);
        if (staged) {
            rot.resize((size_t)rw * rh);
            for (int y = 0; y < rh; ++y)
                for (int x = 0; x < rw; ++x) rot[(size_t)y * rw + x] = rot_px(fr, g, rx0 + x, ry0 + y);
        }
        for (int oy = 0; oy < out_h; ++oy) {
            const Ent ey = extent_entry(g.box[1], g.box[3], out_h, oy, g.H);
            for (int ox = 0; ox < out_w; ++ox) {
                const Ent ex = extent_entry(g.box[0], g.box[2], out_w, ox, g.W);
                uint8_t v = 0;
                if (ex.i != kOutside && ey.i != kOutside) {
                    if (staged)
                        // (the clamps change nothing for a geom of normalize_geometry_host; a hand-made rect cannot make a tap leave the buffer)
                        v = sample([&](int xc, int yc) { return (double)rot[(size_t)clip(yc - ry0, rh) * rw + clip(xc - rx0, rw)]; }, ex.i, ex.d, ey.i, ey.d, g.W,
                                   g.H);
                    else
                        v = sample([&](int xc, int yc) { return (double)rot_px(fr, g, xc, yc); }, ex.i, ex.d, ey.i, ey.d, g.W, g.H);
                }
                dst[(size_t)oy * out_w + ox] = v;
            }
        }
    }
    return nullptr;
}

}  // namespace hg
