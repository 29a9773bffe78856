/* Stand-in for <pangolin/pangolin.h>: Map.h names one OpenGL type for a thumbnail that nothing here touches. */
#ifndef REF_CAM_SHIM_PANGOLIN_H
#define REF_CAM_SHIM_PANGOLIN_H
typedef unsigned char GLubyte;
namespace pangolin { struct GlTexture; struct OpenGlMatrix; }
#endif
