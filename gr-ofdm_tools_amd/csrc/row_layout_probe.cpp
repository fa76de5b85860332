// Host-only probe of csrc/row_layout.h, built on the fly by tests/test_abi_cpu.py::test_row_layouts_are_permutations with
// g++ - NOT part of libofdmtools_hip.so: bin_pos as the finalize kernels call it, and the writers' layout helpers.
#include "row_layout.h"

extern "C" {
int oth_probe_bin_pos(int pos, int layout, int l1, int l2) { return oth::bin_pos(pos, (oth::RowLayout)layout, l1, l2); }
int oth_probe_w16k_layout(int nfft) { return oth::w16k_layout(nfft); }
int oth_probe_x1_layout(int nfft) { return oth::x1_layout(nfft); }
int oth_probe_w32k_layout(int L) { return oth::w32k_layout(L); }
}
