#pragma once
/* What LoopClosing.h declares with: g2o::Sim3 members and a map of them (LoopClosing.h:50-51, :156-199). */
#include <Eigen/Core>
namespace g2o {
class Sim3 {};
class SE3Quat {};
}  // namespace g2o
