#pragma once
#include <opencv2/core/core.hpp>   /* Tracking.h: cv::KalmanFilter is not used by the declarations it reaches */
