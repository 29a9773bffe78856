/* Stand-in for <opencv2/imgproc/imgproc.hpp>: the camera models use nothing of it. */
#ifndef REF_CAM_SHIM_IMGPROC_HPP
#define REF_CAM_SHIM_IMGPROC_HPP
#include "opencv2/core/core.hpp"
#endif
