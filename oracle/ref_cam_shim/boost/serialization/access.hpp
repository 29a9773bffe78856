/* Stand-in for boost::serialization: the camera models only declare serialize() templates, which nothing instantiates. */
#ifndef REF_CAM_SHIM_BOOST_SERIALIZATION
#define REF_CAM_SHIM_BOOST_SERIALIZATION
namespace boost {
namespace serialization {
class access {};
template <typename Base, typename Derived>
Base &base_object(Derived &d) { return d; }
}  // namespace serialization
}  // namespace boost
#endif
