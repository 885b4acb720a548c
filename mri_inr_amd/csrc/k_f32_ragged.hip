// Device code of the siren_trunk_f32_ragged.hip.h instances libmsiren launches (the lists: trunk_instances.h).
#include "siren_trunk_f32_ragged.hip.h"
#include "trunk_instances.h"
namespace msiren {
MSIREN_F32_RAGGED_INSTANCES(MSIREN_DEFINE_TRUNK)
MSIREN_F32_JET_RAGGED_INSTANCES(MSIREN_DEFINE_TRUNK)
MSIREN_F32_RAGGED_COND_INSTANCES(MSIREN_DEFINE_TRUNK)
}  // namespace msiren
