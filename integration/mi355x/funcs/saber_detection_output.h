// saber/funcs/impl/mi355x/saber_detection_output.h — SaberDetectionOutput<MI355X, OpDtype> (facade: saber/funcs/detection_output.h,
// pattern: saber/funcs/impl/x86/saber_detection_output.h). AK_FLOAT runs saber_hip_detout_*: decode, per-class NMS and the keep_top_k cut
// on the device, the output reshaped to the number of kept rows outside an op-list capture and left at its capacity shape inside one
// (INTEGRATION.md). Any other OpDtype, share_location = false, keep_top_k < 1 and nms_top_k outside 1 .. 1024 answer SaberUnImplError.
#ifndef ANAKIN_SABER_FUNCS_IMPL_MI355X_SABER_DETECTION_OUTPUT_H
#define ANAKIN_SABER_FUNCS_IMPL_MI355X_SABER_DETECTION_OUTPUT_H

#include "saber/funcs/impl/impl_detection_output.h"
#include "saber_mi355x_adaptor.h"

namespace anakin {
namespace saber {

template <DataType OpDtype>
class SaberDetectionOutput<MI355X, OpDtype> : public SaberDetectionOutputMI355X<MI355X, OpDtype> {};

}  // namespace saber
}  // namespace anakin
#endif
