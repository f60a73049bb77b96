// The kernel-expression instantiations of the float64 kernelised tile kernel (lketkf_tile64.hip, template parameter ST != 0):
// a translation unit of their own so that they compile beside the RBF instantiations.
#define MIA_KERN64_TU 1
#include "lketkf_tile64.hip"
