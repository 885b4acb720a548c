// Device code of the siren_trunk_f16x3n_ragged_kernel instances libmsiren launches (siren_trunk_f16x3n_ragged.hip.h; the list: trunk_instances.h).
#include "siren_trunk_f16x3n_ragged.hip.h"
#include "trunk_instances.h"
namespace msiren {
MSIREN_F16X3N_RAGGED_INSTANCES(MSIREN_DEFINE_TRUNK)
}  // namespace msiren
