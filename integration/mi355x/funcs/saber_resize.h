// saber/funcs/impl/mi355x/saber_resize.h — SaberResize<MI355X, OpDtype> (facade: saber/funcs/resize.h, pattern:
// saber/funcs/impl/x86/saber_resize.h). AK_FLOAT runs saber_hip_resize_*; any other OpDtype answers SaberUnImplError from create
// (the x86 file instantiates AK_FLOAT alone). One input: the two-input form, where a second tensor carries the output size, is refused.
#ifndef ANAKIN_SABER_FUNCS_IMPL_MI355X_SABER_RESIZE_H
#define ANAKIN_SABER_FUNCS_IMPL_MI355X_SABER_RESIZE_H

#include "saber/funcs/impl/impl_resize.h"
#include "saber_mi355x_adaptor.h"

namespace anakin {
namespace saber {

template <DataType OpDtype>
class SaberResize<MI355X, OpDtype> : public SaberResizeMI355X<MI355X, OpDtype> {};

}  // namespace saber
}  // namespace anakin
#endif
