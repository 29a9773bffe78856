/* Forwarder: everything the reference extractor needs is in the stand-in container header. */
#include "../../opencv/cv.h"
