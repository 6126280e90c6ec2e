// saber/funcs/impl/mi355x/saber_concat.h — SaberConcat<MI355X, OpDtype> (facade: saber/funcs/concat.h,
// pattern: saber/funcs/impl/x86/saber_concat.h)
#ifndef ANAKIN_SABER_FUNCS_IMPL_MI355X_SABER_CONCAT_H
#define ANAKIN_SABER_FUNCS_IMPL_MI355X_SABER_CONCAT_H

#include "saber/funcs/impl/impl_concat.h"
#include "saber_mi355x_adaptor.h"

namespace anakin {
namespace saber {

template <DataType OpDtype>
class SaberConcat<MI355X, OpDtype> : public SaberConcatMI355X<MI355X, OpDtype> {};

}  // namespace saber
}  // namespace anakin
#endif
