#pragma once
/* What Converter.h declares with: g2o::SE3Quat and g2o::Sim3, which the double for types_seven_dof_expmap.h already names. */
#include "Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h"
