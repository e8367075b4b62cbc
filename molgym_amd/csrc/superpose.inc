// superpose.inc -- the RMSD of two sets of canvases after the best translation and proper rotation (include/molgym_hip.h:
// mg_superpose; molgym_amd/structure.py, whose `superpose_host` is the float64 mirror).  Relaxation (relax.inc) tells how much
// energy a molecule drops; how far it moved is this kernel: one workgroup of 256 threads per pair of canvases, one thread per atom
// (thread i owns atom i; with a mask the selected atoms come first).
//
// The operation order IS the interface (+ - * /, comparisons, selects and sqrt only -- `1.0 / sqrt(x)`, no reciprocal square root --
// float64, contraction off).  R is the workgroup reduction of relax.inc (rx_reduce): 256 slots, then v[i] = v[i] + v[i+s] for
// s = 128, 64, ..., 1 (Rmax: the larger of the two, a NaN wins).  The selected atoms of a row fill the slots 0 .. m-1 in atom
// order -- slot k holds the value of the k-th selected atom; without a mask slot i holds atom i's -- and every other slot holds
// +0.0, so a selected subset gives the bits of the subset alone.  Per row with n atoms a_i, b_i, of which m are selected:
//   m = R(selected ? 1.0 : 0.0)
//   m == 0:  rmsd = displacement = max_deviation = 0.0, the rotation is the identity, the centroids are 0.0, the status is OK and
//            `aligned` gets the bytes of B
//   centroids     ca_k = R(a_k) / m, cb_k = R(b_k) / m over the selected atoms;  a' = a - ca, b' = b - cb for every atom of the row
//   displacement  d = a - b;  D = R((dx*dx + dy*dy) + dz*dz);  displacement = sqrt(D / m)
//   covariance    M_kl = R(b'_k * a'_l), nine sums
//   Horn's matrix K00 = (Mxx+Myy)+Mzz  K11 = (Mxx-Myy)-Mzz  K22 = (Myy-Mxx)-Mzz  K33 = (Mzz-Mxx)-Myy
//                 K01 = Myz-Mzy  K02 = Mzx-Mxz  K03 = Mxy-Myx  K12 = Mxy+Myx  K13 = Mzx+Mxz  K23 = Myz+Mzy,  K symmetric
//   cyclic Jacobi a full 4 x 4 working copy A = K and V = I; exactly 8 sweeps over (p,q) = (0,1),(0,2),(0,3),(1,2),(1,3),(2,3).  A
//                 pair whose A_pq == 0.0 is skipped; otherwise
//                   th = (A_qq - A_pp) / (2.0*A_pq);  t = 1.0 / (|th| + sqrt(th*th + 1.0)), negated when th < 0
//                   c = 1.0 / sqrt(t*t + 1.0);  s = t*c
//                   for k = 0..3 the columns  (A_kp, A_kq) <- (c*A_kp - s*A_kq, s*A_kp + c*A_kq)
//                   then for k = 0..3 the rows (A_pk, A_qk) <- (c*A_pk - s*A_qk, s*A_pk + c*A_qk)
//                   then for k = 0..3 the columns of V as those of A
//                 (an overflowing th gives t = 0, a rotation that does nothing: intended)
//   quaternion    j = the first index of the largest A_jj;  v = V[:, j];  q = v / sqrt(((v0*v0 + v1*v1) + v2*v2) + v3*v3), every
//                 component negated when q0 < 0;  (w, x, y, z) = q
//   rotation      R00 = ((w*w + x*x) - y*y) - z*z   R01 = 2.0*(x*y - w*z)             R02 = 2.0*(x*z + w*y)
//                 R10 = 2.0*(x*y + w*z)             R11 = ((w*w - x*x) + y*y) - z*z   R12 = 2.0*(y*z - w*x)
//                 R20 = 2.0*(x*z - w*y)             R21 = 2.0*(y*z + w*x)             R22 = ((w*w - x*x) - y*y) + z*z
//   residuals     rb_k = (R_k0*b'_x + R_k1*b'_y) + R_k2*b'_z;  aligned_k = rb_k + ca_k for every atom of the row, selected or not
//                 res = a' - rb;  r2 = (rx*rx + ry*ry) + rz*rz
//                 rmsd = sqrt(R(selected ? r2 : 0.0) / m);  max_deviation = sqrt(Rmax(selected ? r2 : 0.0))
// The rmsd is taken from the residuals and not from Ga + Gb - 2 lambda, which cancels when the structures nearly coincide.
//
// NONFINITE (m > 0): D is not finite, or one of the 16 entries of A or of the 16 entries of V is not finite after the eighth sweep.
// That test covers every sum in front of it: a non-finite A or V entry stays non-finite under a rotation (c >= 1/sqrt(2) is never 0,
// so c*inf is inf, and inf - x, a NaN and 0*inf are not finite; a NaN c or s reaches every entry of the two columns of V), every
// M_kl is a term of an entry of K, so a non-finite M_kl makes K = A non-finite from the start, and a non-finite centroid component
// makes a'_l or b'_k non-finite for every selected atom, and with it a product of every sum M_kl it enters.  Such a row gets NaN in
// the three scalars, the rotation and the centroids, and `aligned` gets the bytes of B.  A row whose atom count lies outside 0 .. N
// is NONFINITE in the same way, and nothing of it is indexed.  Slots beyond a row's atoms of `aligned` always get the bytes of B.
// A NaN or an infinity in an unselected atom takes no part in any sum: the row is OK and that atom's `aligned` is what the
// arithmetic gives.
//
// LDS: the two arrays of 256 reduction slots of rx_reduce (4 KB), nothing else; the atom, the sums, A and V live in registers.
// Every thread solves the 4 x 4 eigenproblem for itself from the same reduced sums (rx_reduce hands v[0] to every thread), so the
// control flow is uniform and nothing is broadcast.  19 reductions, one barrier each.  Plain vector stores, no atomics.
#pragma once
#include "relax.inc"

struct SuperposeArgs {
  int E, N;
  const double *pos_a, *pos_b;
  const int* natoms;
  const unsigned char* select;  // [E][N] or null
  double *aligned;              // [E][N][3] or null
  double *rmsd, *displacement, *max_deviation, *rotation, *centroid_a, *centroid_b;
  int* status;
};

// one Jacobi rotation of the pair (P, Q): compile-time indices keep A and V in registers
template <int P, int Q>
__device__ __forceinline__ void sp_rotate(double (&A)[4][4], double (&V)[4][4]) {
#pragma clang fp contract(off)
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double th = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  double t = 1.0 / (__builtin_fabs(th) + sqrt(th * th + 1.0));
  if (th < 0.0) t = -t;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double x = A[k][P], y = A[k][Q];
    A[k][P] = c * x - s * y;
    A[k][Q] = s * x + c * y;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double x = A[P][k], y = A[Q][k];
    A[P][k] = c * x - s * y;
    A[Q][k] = s * x + c * y;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double x = V[k][P], y = V[k][Q];
    V[k][P] = c * x - s * y;
    V[k][Q] = s * x + c * y;
  }
}

// what a row without a superposition gets: v in the scalars, the rotation and the centroids (thread 0)
__device__ __forceinline__ void sp_no_fit(const SuperposeArgs& S, int e, double v, double diag, int status) {
  S.rmsd[e] = S.displacement[e] = S.max_deviation[e] = v;
  for (int k = 0; k < 9; ++k) S.rotation[(size_t)e * 9 + k] = (k == 0 || k == 4 || k == 8) ? diag : v;
  for (int k = 0; k < 3; ++k) S.centroid_a[(size_t)e * 3 + k] = S.centroid_b[(size_t)e * 3 + k] = v;
  S.status[e] = status;
}

__global__ __launch_bounds__(RX_T) void k_superpose(SuperposeArgs S) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double red[2 * RX_T];
  const int e = blockIdx.x, i = threadIdx.x, N = S.N;
  const unsigned long long* b_bits = reinterpret_cast<const unsigned long long*>(S.pos_b);
  unsigned long long* out_bits = reinterpret_cast<unsigned long long*>(S.aligned);
  const int n = __builtin_amdgcn_readfirstlane(S.natoms[e]);
  const double nan = __builtin_nan("");
  if (n < 0 || n > N) {  // the whole row is copied, nothing of it is looked at
    if (i < N && S.aligned != nullptr)
      for (int k = 0; k < 3; ++k) out_bits[((size_t)e * N + i) * 3 + k] = b_bits[((size_t)e * N + i) * 3 + k];
    if (i == 0) sp_no_fit(S, e, nan, nan, MG_SUPERPOSE_NONFINITE);
    return;
  }
  // the atom this thread owns: thread i < m owns the i-th selected atom, thread m <= i < n the (i - m)-th unselected one, so the
  // selected atoms fill the slots 0 .. m-1 of every sum in atom order (no mask: thread i owns atom i).  Every wave ballots the
  // mask of all 256 slots for itself -- four uniform 64-bit words, no LDS -- and a thread picks its bit by popcounts.
  int own = i < n ? i : -1, picked = n;
  if (S.select != nullptr) {
    const int lane = i & 63;
    unsigned long long w[4], in[4];
    picked = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = lane + 64 * k;
      w[k] = __ballot(j < n && S.select[(size_t)e * N + j] != 0);
      in[k] = __ballot(j < n);
      picked += __popcll(w[k]);
    }
    int r = i < picked ? i : i - picked;
    own = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned long long bits = i < picked ? w[k] : in[k] & ~w[k];
      const int c = __popcll(bits);
      if (own < 0 && i < n) {
        if (r < c) {
          int pos = 0;  // the r-th set bit of `bits`
#pragma unroll
          for (int width = 32; width >= 1; width >>= 1) {
            const int below = __popcll((bits >> pos) & ((1ull << width) - 1ull));
            if (r >= below) { r -= below; pos += width; }
          }
          own = 64 * k + pos;
        } else {
          r -= c;
        }
      }
    }
  }
  const bool me = own >= 0, sel = me && i < picked;
  // this thread's slot of the canvases: its atom, or slot i beyond the atoms.  B's bytes of it are read before anything is
  // written: `aligned` may be pos_b, and a thread writes only the slot it read
  const size_t at = (size_t)e * N + (me ? own : i);
  unsigned long long bq[3] = {0ull, 0ull, 0ull};
  if (i < N)
    for (int k = 0; k < 3; ++k) bq[k] = b_bits[at * 3 + k];
  double a[3] = {0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
  if (me)
    for (int k = 0; k < 3; ++k) {
      a[k] = S.pos_a[at * 3 + k];
      b[k] = __longlong_as_double((long long)bq[k]);
    }
  int par = 0;
  const double m = rx_reduce<false>(red, par, sel ? 1.0 : 0.0);
  bool fit = m != 0.0;
  double ca[3] = {0.0, 0.0, 0.0}, cb[3] = {0.0, 0.0, 0.0}, rot[3][3], rb[3] = {0.0, 0.0, 0.0}, a1[3], D = 0.0;
  if (fit) {
    double b1[3];
    for (int k = 0; k < 3; ++k) ca[k] = rx_reduce<false>(red, par, sel ? a[k] : 0.0) / m;
    for (int k = 0; k < 3; ++k) cb[k] = rx_reduce<false>(red, par, sel ? b[k] : 0.0) / m;
    for (int k = 0; k < 3; ++k) { a1[k] = a[k] - ca[k]; b1[k] = b[k] - cb[k]; }
    {
      const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      D = rx_reduce<false>(red, par, sel ? d2 : 0.0);
    }
    double M[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int l = 0; l < 3; ++l) {
        const double w = b1[k] * a1[l];
        M[k][l] = rx_reduce<false>(red, par, sel ? w : 0.0);
      }
    double A[4][4], V[4][4];
    A[0][0] = (M[0][0] + M[1][1]) + M[2][2];
    A[1][1] = (M[0][0] - M[1][1]) - M[2][2];
    A[2][2] = (M[1][1] - M[0][0]) - M[2][2];
    A[3][3] = (M[2][2] - M[0][0]) - M[1][1];
    A[0][1] = A[1][0] = M[1][2] - M[2][1];
    A[0][2] = A[2][0] = M[2][0] - M[0][2];
    A[0][3] = A[3][0] = M[0][1] - M[1][0];
    A[1][2] = A[2][1] = M[0][1] + M[1][0];
    A[1][3] = A[3][1] = M[2][0] + M[0][2];
    A[2][3] = A[3][2] = M[1][2] + M[2][1];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int l = 0; l < 4; ++l) V[k][l] = k == l ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < 8; ++sweep) {
      sp_rotate<0, 1>(A, V);
      sp_rotate<0, 2>(A, V);
      sp_rotate<0, 3>(A, V);
      sp_rotate<1, 2>(A, V);
      sp_rotate<1, 3>(A, V);
      sp_rotate<2, 3>(A, V);
    }
    bool finite = rx_finite(D);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int l = 0; l < 4; ++l) finite = finite && rx_finite(A[k][l]) && rx_finite(V[k][l]);
    if (!finite) {
      if (i < N && S.aligned != nullptr)
        for (int k = 0; k < 3; ++k) out_bits[at * 3 + k] = bq[k];
      if (i == 0) sp_no_fit(S, e, nan, nan, MG_SUPERPOSE_NONFINITE);
      return;
    }
    // the column of the first largest diagonal entry, by selects
    double best = A[0][0], v[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const bool up = A[k][k] > best;
      best = up ? A[k][k] : best;
#pragma unroll
      for (int l = 0; l < 4; ++l) v[l] = up ? V[l][k] : v[l];
    }
    const double norm = sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3]);
    double q[4];
    for (int l = 0; l < 4; ++l) q[l] = v[l] / norm;
    if (q[0] < 0.0)
      for (int l = 0; l < 4; ++l) q[l] = -q[l];
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    rot[0][0] = ((w * w + x * x) - y * y) - z * z;
    rot[0][1] = 2.0 * (x * y - w * z);
    rot[0][2] = 2.0 * (x * z + w * y);
    rot[1][0] = 2.0 * (x * y + w * z);
    rot[1][1] = ((w * w - x * x) + y * y) - z * z;
    rot[1][2] = 2.0 * (y * z - w * x);
    rot[2][0] = 2.0 * (x * z - w * y);
    rot[2][1] = 2.0 * (y * z + w * x);
    rot[2][2] = ((w * w - x * x) - y * y) + z * z;
    for (int k = 0; k < 3; ++k) rb[k] = (rot[k][0] * b1[0] + rot[k][1] * b1[1]) + rot[k][2] * b1[2];
  }
  if (i < N && S.aligned != nullptr) {
    if (me && fit)
      for (int k = 0; k < 3; ++k) S.aligned[at * 3 + k] = rb[k] + ca[k];
    else
      for (int k = 0; k < 3; ++k) out_bits[at * 3 + k] = bq[k];
  }
  if (!fit) {
    if (i == 0) sp_no_fit(S, e, 0.0, 1.0, MG_SUPERPOSE_OK);
    return;
  }
  const double rx = a1[0] - rb[0], ry = a1[1] - rb[1], rz = a1[2] - rb[2];
  const double r2 = (rx * rx + ry * ry) + rz * rz;
  const double sum = rx_reduce<false>(red, par, sel ? r2 : 0.0);
  const double top = rx_reduce<true>(red, par, sel ? r2 : 0.0);
  if (i == 0) {
    S.rmsd[e] = sqrt(sum / m);
    S.displacement[e] = sqrt(D / m);
    S.max_deviation[e] = sqrt(top);
    for (int k = 0; k < 9; ++k) S.rotation[(size_t)e * 9 + k] = rot[k / 3][k % 3];
    for (int k = 0; k < 3; ++k) { S.centroid_a[(size_t)e * 3 + k] = ca[k]; S.centroid_b[(size_t)e * 3 + k] = cb[k]; }
    S.status[e] = MG_SUPERPOSE_OK;
  }
}

extern "C" int mg_superpose(int32_t E, int32_t N, const double* pos_a, const double* pos_b, const int32_t* natoms, const uint8_t* select,
                            double* aligned, double* rmsd, double* displacement, double* max_deviation, double* rotation,
                            double* centroid_a, double* centroid_b, int32_t* status, void* stream) {
  const int rc = traj_check_shape("mg_superpose", E, 1, 0, N);
  if (rc != MG_OK) return rc;
  if (!pos_a || !pos_b || !natoms || !rmsd || !displacement || !max_deviation || !rotation || !centroid_a || !centroid_b || !status)
    MG_FAIL(MG_EINVAL, "mg_superpose: null pointer argument");
  if (aligned == pos_a) MG_FAIL(MG_EINVAL, "mg_superpose: aligned may be pos_b, not pos_a");
  SuperposeArgs a;
  a.E = E; a.N = N; a.pos_a = pos_a; a.pos_b = pos_b; a.natoms = natoms; a.select = select; a.aligned = aligned;
  a.rmsd = rmsd; a.displacement = displacement; a.max_deviation = max_deviation; a.rotation = rotation;
  a.centroid_a = centroid_a; a.centroid_b = centroid_b; a.status = status;
  hipLaunchKernelGGL(k_superpose, dim3(E), dim3(RX_T), 0, (hipStream_t)stream, a);
  LAUNCH_CHECK();
  return MG_OK;
}
