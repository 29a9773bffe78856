#pragma once
/* the matcher adapter's double, plus the one name MapDrawer.h adds (MapDrawer.h:42-46) */
#include_next <pangolin/pangolin.h>
namespace pangolin { struct OpenGlMatrix {}; }
