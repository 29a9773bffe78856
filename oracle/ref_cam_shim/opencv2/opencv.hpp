/*
 * Stand-in for <opencv2/opencv.hpp> (TEST INFRASTRUCTURE), reached through the reference's TwoViewReconstruction.h.
 *
 * This is the header that decides the libm overloads of the two camera files.  OpenCV 3.4.6's own headers include <math.h> (its
 * FLANN headers do), and with libstdc++ >= 6 <math.h> is a wrapper that brings std::cos(float), std::sin(float), ... into the global
 * namespace.  The unqualified cos(psi) / sin(psi) of a float inside namespace ORB_SLAM3 (KannalaBrandt8.cpp:42-43) are then the FLOAT
 * overloads.  With <cmath> alone only ::cos(double) is visible there and the same text computes in double.
 * -DREF_CAM_SHIM_CMATH builds that second reading (libref_cameras_cmath.so, for the one test that tells the two apart).
 */
#ifndef REF_CAM_SHIM_OPENCV_HPP
#define REF_CAM_SHIM_OPENCV_HPP
#ifdef REF_CAM_SHIM_CMATH
#include <cmath>
#else
#include <math.h>
#endif
#include "opencv2/core/core.hpp"
#endif
