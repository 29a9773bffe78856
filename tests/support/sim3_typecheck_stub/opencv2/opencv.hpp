/* Put in front of the other doubles for translation units that begin with Sim3Solver.h: Map.h (reached through KeyFrame.h) names `list`
 * without including <list>, which the real opencv2/opencv.hpp brings along.  Only that; the rest is the next double's. */
#pragma once
#include <list>
#include_next <opencv2/opencv.hpp>
