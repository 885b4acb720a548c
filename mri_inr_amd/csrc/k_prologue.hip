// Device code of the encoder_modulator_f16x3.hip.h instances libmsiren launches (the list: trunk_instances.h).
#include "encoder_modulator_f16x3.hip.h"
#include "trunk_instances.h"
namespace msiren {
MSIREN_PROLOGUE_INSTANCES(MSIREN_DEFINE_PROLOGUE)
}  // namespace msiren
