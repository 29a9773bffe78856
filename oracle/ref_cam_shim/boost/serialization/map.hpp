/* Stand-in for boost::serialization: see serialization.hpp. */
#include "serialization.hpp"
