/* Stand-in for <opencv2/features2d/features2d.hpp>: cv::KeyPoint is in core.hpp; the camera models use nothing else of it. */
#ifndef REF_CAM_SHIM_FEATURES2D_HPP
#define REF_CAM_SHIM_FEATURES2D_HPP
#include "opencv2/core/core.hpp"
#endif
