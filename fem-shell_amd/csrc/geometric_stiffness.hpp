// geometric_stiffness.hpp -- launchers of the geometric (initial-stress) stiffness K_G(N) (geometric_stiffness.hip; DESIGN.md 8g;
// femshell_geometric_product).  K_G is never stored as a matrix: a block of it is one scalar g_ab times I3 on the translations, so
// an element keeps the 6 (TRI3) or 10 (a mesh with QUAD4) unique g_ab and the product walks the slices' element lists.
#pragma once

#include "kernels.hpp"

namespace femshell {

constexpr int kGeoMaxCols = 4; // columns one pass of the product multiplies
// doubles per element in the coefficient array: the upper triangle of g, row by row -- 3 x 3 on a mesh of triangles, 4 x 4 (a
// triangle's fourth row and column zero) where the mesh has quadrilaterals.  Rows are whole 16-byte words.
inline int geometric_coeff_words(const DeviceMatrix &m) { return m.n_lquad > 0 ? 10 : 6; }

// coeff[(n_ltri + n_lquad)][6 | 10], LOCAL element order, from the rows launch_element_resultants left at `res` (14 doubles per
// element, the first six the membrane force tensor N in global axes).  One lane per element, no atomics.  A degenerate element
// writes zeros and reports kStatusDirect + its index through m.status.
void launch_geometric_coeff(const DeviceMatrix &m, const double *res, double *coeff, hipStream_t st);

// Y = K_G X, n_cols columns (column j at X + j * ld, Y + j * ld; ld >= (n_pad + n_ghost) * 6): the translations of the owned rows
// get sum over the row's elements, in the order of the slice's list, of sum_b g_ab x_b; the rotations, the padding rows and the
// ghost space get zero.  solver: Y = -K_G X on the free dofs and zero on the constrained ones (m.dmask) instead.  ceil(n_cols / 4)
// passes of four columns and a narrower tail; column j is bitwise the single-column product; no atomics: two launches give the
// same bits at every grid size.  Y must not alias X.
void launch_geometric_product(const DeviceMatrix &m, const int32_t *slice_elem_local, const double *coeff, const double *X, double *Y,
                              int64_t ld, int n_cols, bool solver, hipStream_t st);

} // namespace femshell
