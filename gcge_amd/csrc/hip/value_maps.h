// Where the stored values of the star and the dense forms come from (kept on request: gcge_hip_mat_keep_value_maps) and the rule that
// replays that provenance on new values — shared by the host builders (star_split.hip, spmm_dense.hip), the host self-check and the
// update kernels (mat_values_forms.hip), the way pattern_table.h shares the slot rule.
//   a map entry    index into the builder's input array of values, -1: no source (padding, a row without a diagonal, an entry the split
//                  "takes back" where the row has none)
//   a code         0: none; otherwise the star coefficient of axis a (0 x, 1 y, 2 z) and distance k (1 .. GCGE_VM_ARM): the stored value
//                  is the gathered one MINUS that coefficient, rounded once (star_build_host)
//   a pin          per CSR entry: the code of the coefficient the entry equalled at creation (it sits at a star position and has no
//                  remainder slot: new values must keep it, bit for bit), GCGE_VM_PIN_DIAG for the row's diagonal entry (no NaN), 0: free
#ifndef GCGE_VALUE_MAPS_H
#define GCGE_VALUE_MAPS_H
#if defined(__HIPCC__)
#define GCGE_VM_HD __host__ __device__
#else
#define GCGE_VM_HD
#endif

#define GCGE_VM_ARM 6                             // = gcge::STAR_R (star_split.hip asserts it)
#define GCGE_VM_NCODE (1 + 3 * GCGE_VM_ARM)
#define GCGE_VM_PIN_DIAG 255
struct GcgeVmCoef { double c[GCGE_VM_NCODE]; };   // [code]; [0] unused

GCGE_VM_HD static inline int gcge_vm_code(int axis, int k) { return 1 + axis * GCGE_VM_ARM + (k - 1); }
// gather: blocks, pad-8 slots, the star's diagonal
GCGE_VM_HD static inline double gcge_vm_gather(const double* v, int idx) { return idx >= 0 ? v[idx] : 0.0; }
// gather minus coefficient: the star's remainder
GCGE_VM_HD static inline double gcge_vm_replay(const double* v, int idx, int code, const double* coef) {
  if (code == 0) return gcge_vm_gather(v, idx);
  return idx >= 0 ? v[idx] - coef[code] : -coef[code];
}
// the check of one CSR entry before anything is written: 0 fine, 1 a pinned entry differs from its coefficient, 2 a NaN on the diagonal
GCGE_VM_HD static inline int gcge_vm_check(double v, int pin, const double* coef) {
  if (pin == 0) return 0;
  if (pin == GCGE_VM_PIN_DIAG) return v != v ? 2 : 0;
  union { double d; unsigned long long u; } a, b;
  a.d = v; b.d = coef[pin];
  return a.u != b.u ? 1 : 0;
}
#endif
