// saber/funcs/impl/mi355x/saber_deconv.h — SaberDeconv2D<MI355X, OpDtype> (facade: saber/funcs/deconv.h:47-125,
// pattern: saber/funcs/impl/x86/saber_deconv.h). AK_FLOAT runs saber_hip_deconv2d_*; AK_INT8 answers SaberUnImplError from
// create, as the x86 specialisation does (saber/funcs/impl/x86/saber_deconv.cpp:66-76).
#ifndef ANAKIN_SABER_FUNCS_IMPL_MI355X_SABER_DECONV_H
#define ANAKIN_SABER_FUNCS_IMPL_MI355X_SABER_DECONV_H

#include "saber/funcs/impl/impl_deconv.h"
#include "saber_mi355x_adaptor.h"

namespace anakin {
namespace saber {

template <DataType OpDtype>
class SaberDeconv2D<MI355X, OpDtype> : public SaberDeconv2DMI355X<MI355X, OpDtype> {};

}  // namespace saber
}  // namespace anakin
#endif
