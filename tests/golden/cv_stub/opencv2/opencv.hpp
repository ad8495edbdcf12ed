// OpenCV stand-in for tests/golden/make_segment_golden.py: just enough of the API for the reference's
// selectScanPoints.cpp to compile and for AutoGetLinePts to run headless.  Drawing and windows are no-ops.
#pragma once
#include <string>
#include <vector>
typedef unsigned char uchar;
#define CV_8UC1 0
#define CV_8UC3 16
#define CV_AA 16
namespace cv {
enum { FONT_HERSHEY_COMPLEX_SMALL = 5, EVENT_MOUSEMOVE = 0, EVENT_LBUTTONDOWN = 1, EVENT_LBUTTONUP = 4 };
struct Scalar {
  double v[4];
  Scalar(double a = 0, double b = 0, double c = 0, double d = 0) : v{a, b, c, d} {}
  static Scalar all(double a) { return Scalar(a, a, a, a); }
};
struct Point { int x = 0, y = 0; Point(int a = 0, int b = 0) : x(a), y(b) {} };
struct Rect { int x = 0, y = 0, width = 0, height = 0; };
struct Vec3b { uchar v[3]; Vec3b(uchar a = 0, uchar b = 0, uchar c = 0) : v{a, b, c} {} };
struct Mat {
  int rows = 0, cols = 0;
  std::vector<uchar> data;
  Mat() {}
  Mat(int r, int c, int type, Scalar) : rows(r), cols(c), data((size_t)r * c * (type == CV_8UC3 ? 3 : 1)) {}
  template <class T> T& at(int r, int c) { return *reinterpret_cast<T*>(&data[((size_t)r * cols + c) * sizeof(T)]); }
  Mat clone() const { return *this; }
};
typedef void (*MouseCallback)(int, int, int, int, void*);
inline void imshow(const std::string&, const Mat&) {}
inline int waitKey(int = 0) { return -1; }
inline void namedWindow(const std::string&, int = 0) {}
inline void setMouseCallback(const std::string&, MouseCallback, void* = nullptr) {}
inline void rectangle(Mat&, const Rect&, const Scalar&) {}
inline void putText(Mat&, const std::string&, Point, int, double, Scalar, int = 1, int = 8) {}
}  // namespace cv
inline cv::Point cvPoint(int x, int y) { return cv::Point(x, y); }
inline cv::Scalar cvScalar(double a, double b = 0, double c = 0, double d = 0) { return cv::Scalar(a, b, c, d); }
