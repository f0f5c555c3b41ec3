/* TEST INFRASTRUCTURE ONLY -- stand-in for the slice of OpenCV 3.4 that the reference
 * rasteriser uses (see SDL.h next to this file).
 *
 * imread does not decode JPEG.  It loads "<path>.bgr": three int32 (rows, cols, channels) and
 * then the raw texels, which tests/golden/make_ref_sessions.py writes from oracle.jpeg_decode.
 * The texel VALUES are therefore the oracle's own decode and no independent evidence.  What the
 * unmodified reference does with them is independent: findU / findV, the normal maps, the
 * opacity skip, the first-fragment 0.15 quirk among opaque texels, and the 3 x rows x cols
 * rand() calls of the marble noise loop.  A missing file gives an empty Mat, as OpenCV does.
 */
#ifndef CG_REF_SHIM_CV_HPP
#define CG_REF_SHIM_CV_HPP

#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

typedef unsigned char uchar;

#define CV_LOAD_IMAGE_UNCHANGED (-1)
#define CV_BGR2GRAY 6

namespace cv {

struct Vec3b {
    uchar val[3];
    uchar &operator[](int i) { return val[i]; }
    const uchar &operator[](int i) const { return val[i]; }
};

class Mat {
public:
    int rows, cols;
    Mat() : rows(0), cols(0), channels_(0) {}
    Mat(int r, int c, int ch) : rows(r), cols(c), channels_(ch), data_((size_t)r * c * ch) {}
    bool empty() const { return data_.empty(); }
    int channels() const { return channels_; }
    uchar *ptr() { return data_.data(); }
    const uchar *ptr() const { return data_.data(); }
    /* OpenCV's addressing: the row step is in bytes of the Mat's own element, the column is
     * scaled by sizeof(T) -- so at<uchar> on a 3-channel Mat (the reference's ambient-occlusion
     * read) lands on byte c of the row, not on pixel c.  No bounds check, as in a release build. */
    template <class T> T &at(int r, int c) { return ((T *)(data_.data() + (size_t)r * cols * channels_))[c]; }
private:
    int channels_;
    std::vector<uchar> data_;
};

static inline Mat imread(const std::string &path, int)
{
    FILE *f = fopen((path + ".bgr").c_str(), "rb");
    if (!f)
        return Mat();
    int32_t hdr[3];
    if (fread(hdr, 4, 3, f) != 3 || hdr[0] <= 0 || hdr[1] <= 0 || (hdr[2] != 1 && hdr[2] != 3)) {
        fclose(f);
        return Mat();
    }
    Mat m(hdr[0], hdr[1], hdr[2]);
    const size_t n = (size_t)hdr[0] * hdr[1] * hdr[2];
    const size_t got = fread(m.ptr(), 1, n, f);
    fclose(f);
    return got == n ? m : Mat();
}

/* 8-bit BGR -> gray as OpenCV 3.4 computes it: fixed point, 14 fractional bits, rounded. */
static inline void cvtColor(const Mat &src, Mat &dst, int)
{
    Mat g(src.rows, src.cols, 1);
    const uchar *s = src.ptr();
    uchar *d = g.ptr();
    const size_t n = (size_t)src.rows * src.cols;
    if (src.channels() == 3)
        for (size_t i = 0; i < n; ++i)
            d[i] = (uchar)((s[3 * i] * 1868 + s[3 * i + 1] * 9617 + s[3 * i + 2] * 4899 + (1 << 13)) >> 14);
    else
        for (size_t i = 0; i < n; ++i)
            d[i] = s[i];
    dst = g;
}

/* THRESH_BINARY (type 0) on 8-bit data. */
static inline double threshold(const Mat &src, Mat &dst, double thresh, double maxval, int)
{
    Mat t(src.rows, src.cols, 1);
    const uchar *s = src.ptr();
    uchar *d = t.ptr();
    const size_t n = (size_t)src.rows * src.cols;
    const int th = (int)thresh;
    for (size_t i = 0; i < n; ++i)
        d[i] = s[i] > th ? (uchar)maxval : 0;
    dst = t;
    return thresh;
}

}  // namespace cv

#endif
