// Device code of the siren_trunk_x1w.hip.h instances libmsiren launches (the list: trunk_instances.h).
#include "siren_trunk_x1w.hip.h"
#include "trunk_instances.h"
namespace msiren {
MSIREN_X1W_INSTANCES(MSIREN_DEFINE_TRUNK)
}  // namespace msiren
