// Pillow's Image.resize((w, h), filter) for 8-bit images, restated from Resample.c (ImagingResample): the coefficient tables of one axis
// and the two integer passes on the host.  Plain C++ without HIP, compiled with contraction off and no function multiversioning: every
// double operation below rounds on its own, as Pillow's C does, and sin / cos are the host libm's — the library Pillow itself calls on
// the machine this runs on.  Everything after the tables is integer.
//
// resize is NOT transform(EXTENT, filter) (hg_extract.hip, enum hg_filter): that one samples a fixed 2 x 2 / 4 x 4 neighbourhood of the
// source point; this one is a separable convolution whose support grows with the shrink factor (the antialiasing), with 22-bit fixed
// point coefficients and a uint8 intermediate image between the horizontal and the vertical pass.
#include "hg_resample.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "hg_frame_format.hpp"

namespace hg {

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;
constexpr double kPi = 3.14159265358979323846;      // M_PI

double f_box(double x) { return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0; }
double f_bilinear(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}
double f_hamming(double x) {
    if (x < 0.0) x = -x;
    if (x == 0.0) return 1.0;
    if (x >= 1.0) return 0.0;
    x = x * kPi;
    return std::sin(x) / x * (0.54f + 0.46f * std::cos(x));      // (Pillow writes the two constants as floats)
}
double f_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
double f_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * kPi;
    return std::sin(x) / x;
}
double f_lanczos(double x) { return (-3.0 <= x && x < 3.0) ? f_sinc(x) * f_sinc(x / 3) : 0.0; }

typedef double (*filter_fn)(double);
bool filter_of(int code, filter_fn& f, double& support) {
    switch (code) {
        case HG_RESAMPLE_BOX: f = f_box; support = 0.5; return true;
        case HG_RESAMPLE_BILINEAR: f = f_bilinear; support = 1.0; return true;
        case HG_RESAMPLE_HAMMING: f = f_hamming; support = 1.0; return true;
        case HG_RESAMPLE_BICUBIC: f = f_bicubic; support = 2.0; return true;
        case HG_RESAMPLE_LANCZOS: f = f_lanczos; support = 3.0; return true;
        default: return false;
    }
}

inline uint8_t clip8(uint32_t acc) {
    const int32_t v = (int32_t)acc >> kPrecisionBits;      // arithmetic shift, as Pillow's clip8
    return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// one pass along a line of n_out elements: element e = (pixel e / C, band e % C) reads source bytes (xmin + x) * C + band
// (`first`: the source index src[0] stands for)
void pass_line(const uint8_t* src, int64_t src_step, const ResampleAxis& ax, int out_index, uint8_t* dst, int first = 0) {
    const int xmin = ax.bounds[2 * out_index] - first, xmax = ax.bounds[2 * out_index + 1];
    const int32_t* k = ax.k.data() + (size_t)out_index * ax.ksize;
    uint32_t acc = 1u << (kPrecisionBits - 1);      // unsigned: Pillow's int sum, with wrap-around defined
    for (int x = 0; x < xmax; ++x) acc += (uint32_t)src[(int64_t)(xmin + x) * src_step] * (uint32_t)k[x];
    *dst = clip8(acc);
}

// PIL's NEAREST resize is the EXTENT rule over the whole frame (hg_extract.hip): a = in / out, o = a / 2, then o += a per output pixel
void nearest_table(int in, int out, std::vector<int32_t>& t) {
    t.resize((size_t)out);
    const double a = (double)in / out;
    double o = 0.0 + a * 0.5;
    for (int i = 0; i < out; ++i, o = o + a) {
        const int v = o < 0.0 ? -1 : (int)o;
        t[(size_t)i] = (v >= 0 && v < in) ? v : -1;
    }
}

}  // namespace

const char* resample_axis(int in, int out, int filter, ResampleAxis& ax) {
    filter_fn f = nullptr;
    double S = 0.0;
    if (!filter_of(filter, f, S)) return "unknown resize filter (1 LANCZOS, 2 BILINEAR, 3 BICUBIC, 4 BOX, 5 HAMMING)";
    if (in <= 0 || out <= 0) return "resize: sizes must be positive";
    double scale = (double)in / out, filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = S * filterscale;
    const double ks = std::ceil(support) * 2 + 1;
    if (ks * (double)out * 4.0 + (double)out * 8.0 > (double)HG_RESAMPLE_MAX_TABLE_BYTES) return "resize: coefficient tables beyond HG_RESAMPLE_MAX_TABLE_BYTES";
    const int ksize = (int)std::ceil(support) * 2 + 1;
    ax.in = in; ax.out = out; ax.filter = filter; ax.ksize = ksize;
    ax.bounds.assign((size_t)out * 2, 0);
    ax.k.assign((size_t)out * ksize, 0);
    std::vector<double> w((size_t)ksize);
    for (int xx = 0; xx < out; ++xx) {
        const double center = 0.0 + (xx + 0.5) * scale;
        const double ss = 1.0 / filterscale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            w[(size_t)x] = f((x + xmin - center + 0.5) * ss);
            ww += w[(size_t)x];
        }
        int32_t* k = ax.k.data() + (size_t)xx * ksize;
        for (int x = 0; x < xmax; ++x) {
            double v = w[(size_t)x];
            if (ww != 0.0) v /= ww;
            k[x] = v < 0 ? (int32_t)(-0.5 + v * (1 << kPrecisionBits)) : (int32_t)(0.5 + v * (1 << kPrecisionBits));
        }
        ax.bounds[(size_t)xx * 2] = xmin;
        ax.bounds[(size_t)xx * 2 + 1] = xmax;
    }
    return nullptr;
}

// Image.resize (Image.py) shrinks the height of a very tall image first — `if self.size[1] > self.size[0] * 100 and size[1] < self.size[1]` —
// and resizes the width of that result afterwards: the intermediate image is another one, so the bytes are others
bool resize_vertical_first(int h, int w, int out_h) { return (int64_t)h > (int64_t)w * 100 && out_h < h; }

const char* resize_check(int filter, const void* src, int format, int h, int w, int64_t ld_bytes, int out_format, const void* dst, int out_h, int out_w,
                         int64_t dst_ld_bytes) {
    if (filter < HG_RESAMPLE_NEAREST || filter > HG_RESAMPLE_HAMMING) return "unknown resize filter (0 NEAREST, 1 LANCZOS, 2 BILINEAR, 3 BICUBIC, 4 BOX, 5 HAMMING)";
    const int bpp = frame_bpp(format);
    if (!bpp) return "unknown frame format (0 L, 1 RGB, 2 BGR, 3 RGBA, 4 BGRA)";
    if (out_format != HG_FRAME_L && out_format != format) return "resize: the output format is HG_FRAME_L or the source's own";
    if (!src || !dst) return "null data pointer";
    if (h <= 0 || w <= 0 || out_h <= 0 || out_w <= 0) return "resize: sizes must be positive";
    const int obpp = frame_bpp(out_format);
    if (ld_bytes < (int64_t)w * bpp) return "bad frame geometry: row stride below the row's bytes";
    if (dst_ld_bytes < (int64_t)out_w * obpp) return "bad output row stride";
    if (filter == HG_RESAMPLE_NEAREST && out_format != HG_FRAME_L) return "resize: NEAREST writes a grey image only";
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)((int64_t)(h - 1) * ld_bytes + (int64_t)w * bpp);
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)((int64_t)(out_h - 1) * dst_ld_bytes + (int64_t)out_w * obpp);
    if (s0 < d1 && d0 < s1) return "resize: source and destination overlap";
    return nullptr;
}

const char* frame_resize_host(int filter, const void* src_v, int format, int h, int w, int64_t ld_bytes, int out_format, void* dst_v, int out_h, int out_w,
                              int64_t dst_ld_bytes) {
    if (const char* why = resize_check(filter, src_v, format, h, w, ld_bytes, out_format, dst_v, out_h, out_w, dst_ld_bytes)) return why;
    const uint8_t* src = (const uint8_t*)src_v;
    uint8_t* dst = (uint8_t*)dst_v;
    const int bpp = frame_bpp(format);
    const bool to_gray = out_format == HG_FRAME_L && format != HG_FRAME_L;
    const bool bgr = format == HG_FRAME_BGR || format == HG_FRAME_BGRA;
    const int C = out_format == HG_FRAME_L ? 1 : bpp;      // bands of the images the passes see
    // a source row as the passes read it: grey rows are converted first, pixel by pixel (im.convert("L").resize(...), the reference's order)
    std::vector<uint8_t> gray;
    auto src_row = [&](int y) -> const uint8_t* {
        const uint8_t* s = src + (int64_t)y * ld_bytes;
        if (!to_gray) return s;
        gray.resize((size_t)w);
        for (int x = 0; x < w; ++x, s += bpp) gray[(size_t)x] = rgb_to_gray(s[bgr ? 2 : 0], s[1], s[bgr ? 0 : 2]);
        return gray.data();
    };
    if (filter == HG_RESAMPLE_NEAREST) {
        std::vector<int32_t> tx, ty;
        nearest_table(w, out_w, tx);
        nearest_table(h, out_h, ty);
        for (int y = 0; y < out_h; ++y) {
            uint8_t* d = dst + (int64_t)y * dst_ld_bytes;
            const int ys = ty[(size_t)y];
            const uint8_t* s = src + (int64_t)(ys >= 0 ? ys : 0) * ld_bytes;
            for (int x = 0; x < out_w; ++x) {
                const int xs = tx[(size_t)x];
                if (xs < 0 || ys < 0) d[x] = 0;
                else if (!to_gray) d[x] = s[xs];
                else d[x] = rgb_to_gray(s[(int64_t)xs * bpp + (bgr ? 2 : 0)], s[(int64_t)xs * bpp + 1], s[(int64_t)xs * bpp + (bgr ? 0 : 2)]);
            }
        }
        return nullptr;
    }
    const bool need_h = out_w != w, need_v = out_h != h;
    if (need_h && resize_vertical_first(h, w, out_h)) {      // Image.resize's own exception: the height first, at full width, then the width
        std::vector<uint8_t> tall((size_t)out_h * (size_t)w * (size_t)C);
        if (const char* why = frame_resize_host(filter, src_v, format, h, w, ld_bytes, out_format, tall.data(), out_h, w, (int64_t)w * C)) return why;
        return frame_resize_host(filter, tall.data(), out_format, out_h, w, (int64_t)w * C, out_format, dst_v, out_h, out_w, dst_ld_bytes);
    }
    ResampleAxis ah, av;
    if (need_h)
        if (const char* why = resample_axis(w, out_w, filter, ah)) return why;
    if (need_v)
        if (const char* why = resample_axis(h, out_h, filter, av)) return why;
    const int64_t n = (int64_t)out_w * C;      // bytes of an output row
    if (!need_h && !need_v) {
        for (int y = 0; y < h; ++y) memcpy(dst + (int64_t)y * dst_ld_bytes, src_row(y), (size_t)n);
        return nullptr;
    }
    // the horizontal pass over the source rows the vertical pass reads (all of them when there is none), into a uint8 image
    const int y_first = need_v ? av.bounds[0] : 0;
    const int y_last = need_v ? av.bounds[(size_t)out_h * 2 - 2] + av.bounds[(size_t)out_h * 2 - 1] : h;
    std::vector<uint8_t> tmp;
    if (need_v) tmp.resize((size_t)(y_last - y_first) * (size_t)n);
    for (int y = y_first; y < y_last; ++y) {
        const uint8_t* s = src_row(y);
        uint8_t* d = need_v ? tmp.data() + (size_t)(y - y_first) * (size_t)n : dst + (int64_t)y * dst_ld_bytes;
        if (!need_h) {
            memcpy(d, s, (size_t)n);
            continue;
        }
        for (int xx = 0; xx < out_w; ++xx)
            for (int b = 0; b < C; ++b) pass_line(s + b, C, ah, xx, d + (int64_t)xx * C + b);
    }
    if (!need_v) return nullptr;
    for (int yy = 0; yy < out_h; ++yy) {
        uint8_t* d = dst + (int64_t)yy * dst_ld_bytes;
        for (int64_t e = 0; e < n; ++e) pass_line(tmp.data() + e, n, av, yy, d + e, y_first);
    }
    return nullptr;
}

}  // namespace hg
