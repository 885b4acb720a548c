// Device code of the siren_trunk_f32_jet.hip.h instances libmsiren launches (the list: trunk_instances.h).
#include "siren_trunk_f32_jet.hip.h"
#include "trunk_instances.h"
namespace msiren {
MSIREN_F32_JET_INSTANCES(MSIREN_DEFINE_TRUNK)
}  // namespace msiren
