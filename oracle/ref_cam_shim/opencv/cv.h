/* Stand-in for <opencv/cv.h>, reached through the reference's ORBextractor.h. */
#include "opencv2/opencv.hpp"
