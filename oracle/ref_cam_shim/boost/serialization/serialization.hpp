/* Stand-in for boost::serialization: the camera models and the SLAM headers only declare serialize() templates, which nothing
   instantiates.  Every boost/serialization/ header of this directory forwards here. */
#ifndef REF_CAM_SHIM_BOOST_SERIALIZATION
#define REF_CAM_SHIM_BOOST_SERIALIZATION
#include <stddef.h>
namespace boost {
namespace serialization {
class access {};
template <typename Base, typename Derived>
Base &base_object(Derived &d) { return d; }
/* named inside the serializeMatrix() templates of the SLAM headers */
template <typename T> struct array_stand_in { T *p; size_t n; };
template <typename T> array_stand_in<T> make_array(T *p, size_t n) { array_stand_in<T> a = {p, n}; return a; }
}  // namespace serialization
}  // namespace boost
#define BOOST_SERIALIZATION_SPLIT_MEMBER()
#define BOOST_SERIALIZATION_ASSUME_ABSTRACT(x)
#define BOOST_CLASS_EXPORT_KEY(x)
#define BOOST_CLASS_EXPORT_IMPLEMENT(x)
#endif
