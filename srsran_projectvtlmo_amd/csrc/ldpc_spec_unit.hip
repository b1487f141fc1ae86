/*
 * Specialised decoder kernels of one unit of ldpc_spec.h's unit table, compiled once per unit letter
 * (-DLDPC_SPEC_UNIT=<letter>, the Makefile's SPEC_UNITS) so that the unrolled kernels compile in parallel.
 * ldpc_hip_kernels.hip's launch_decode reaches them through spec_kernel_<id>() (the host launch stub of
 * ldpc_decode_kernel<true, id>), and its split-row address table writer through spec_split_kernel_<id>().
 */
#ifndef LDPC_SPEC_UNIT
#error "compile with -DLDPC_SPEC_UNIT=<unit letter of ldpc_spec.h>"
#endif
#define LDPC_SPEC_TU_GRAPHS(X) LDPC_SPEC_UNIT_GRAPHS(LDPC_SPEC_UNIT, X)
#include "ldpc_decode_cb.h"
#include "ldpc_hip_launch.h"

namespace ldpc_hip {

#define LDPC_SPEC_KERNEL_DEF(id, bg, z, ils)                                                                           \
  const void* spec_kernel_##id() { return reinterpret_cast<const void*>(&ldpc_decode_kernel<true, id>); }           \
  const void* spec_split_kernel_##id() { return reinterpret_cast<const void*>(&ldpc_split_table_kernel<id>); }
LDPC_SPEC_TU_GRAPHS(LDPC_SPEC_KERNEL_DEF)
#undef LDPC_SPEC_KERNEL_DEF

/* the persistent work-queue kernels of this unit's graphs (ldpc_hip_dwq.cpp): dwq_kernel_<letter> */
#define LDPC_SPEC_UNIT_NAME_(prefix, u) prefix##u
#define LDPC_SPEC_UNIT_NAME(prefix, u) LDPC_SPEC_UNIT_NAME_(prefix, u)
LDPC_DWQ_KERNELS(LDPC_SPEC_UNIT_NAME(dwq_kernel_, LDPC_SPEC_UNIT), LDPC_SPEC_TU_GRAPHS)
LDPC_DIAG_UNIT_READER(LDPC_SPEC_UNIT)

} // namespace ldpc_hip
