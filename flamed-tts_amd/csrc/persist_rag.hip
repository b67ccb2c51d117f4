// The exact-lengths ("ragged") variants of the persistent solve, den_persist_kernel<false, NTW, RK2, true>
// (pk::Params::lens): the kernel source of persist.hip compiled once more in a translation unit of its own, which
// instantiates those sixteen variants and nothing else, so they build in parallel with the dense ones and the dense
// object code is what it was.  persist.hip's host side picks them up through pk::persist_ragged_kernel.
#define FL_PERSIST_RAGGED_TU
#include "persist.hip"
