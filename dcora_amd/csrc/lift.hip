// The two images a saddle escape into the next rank starts from (ref src/QuadraticProblem.cpp:148-160), formed on the
// device so that the point never crosses to the host: from X, r x k column-major, and the eigenvector v
//   Xplus (r + 1) x k : column j = [x_j; 0]          the point, one zero row appended
//   dir   (r + 1) x k : column j = [0;  v_col(j)]    the descent direction, v in the new row
// Both orderings (SE: pose by pose, RA: rotations | spheres | translations | landmarks) are the same column walk.
// The whole-graph form reads v where it reads X (col(j) = j).  The agent form (a rank of a job lifts the blocks of the
// agents it hosts, Exchange::lift) reads the GLOBAL v through the agent's column map: a contiguous range that starts at
// col0 (a pose-graph agent), or the agent's list of global columns (a range-aided agent: its rotations, spheres,
// translations and landmarks lie scattered through the global RA ordering).
#include "kernels.h"

#include <cstdint>

namespace dcora {

namespace {

// One pass, both images.  The leading dimension grows from 8 r to 8 (r + 1) bytes, so column j of an image starts at
// 8 (r + 1) j bytes: 16-byte aligned for even (r + 1) j only.  The walk is therefore over PAIRS of the image's linear
// index, not over columns: pair p holds elements 2 p and 2 p + 1, always 16-byte aligned when the image's base is
// (wide), whichever column or columns they fall into -- one 16-byte store per image and lane, consecutive lanes on
// consecutive pairs.  An odd (r + 1) k leaves one last element on its own: it is stored narrow, and nothing of a column
// k is read.  Images whose base is not 16-byte aligned take narrow stores throughout.
__global__ __launch_bounds__(kBlock) void k_lift_images(int r, long k, const double *__restrict__ X,
                                                        const double *__restrict__ v, const int *__restrict__ cols,
                                                        long col0, double *__restrict__ Xplus,
                                                        double *__restrict__ dir, int wide) {
  const int rn = r + 1;
  const long total = (long)rn * k, npairs = (total + 1) / 2;
  for (long p = (long)blockIdx.x * kBlock + threadIdx.x; p < npairs; p += (long)gridDim.x * kBlock) {
    double x[2] = {0.0, 0.0}, w[2] = {0.0, 0.0};
    const int have = (2 * p + 1 < total) ? 2 : 1;
    for (int h = 0; h < have; ++h) {
      const long e = 2 * p + h, j = e / rn;
      const int t = (int)(e - j * rn);
      if (t < r)
        x[h] = X[j * r + t];
      else
        w[h] = v[cols ? (long)cols[j] : col0 + j];
    }
    if (have == 2 && wide) {
      *reinterpret_cast<double2 *>(Xplus + 2 * p) = make_double2(x[0], x[1]);
      *reinterpret_cast<double2 *>(dir + 2 * p) = make_double2(w[0], w[1]);
    } else {
      for (int h = 0; h < have; ++h) {
        Xplus[2 * p + h] = x[h];
        dir[2 * p + h] = w[h];
      }
    }
  }
}

}  // namespace

void launch_lift_images_agent(hipStream_t st, int r, long k, const double *X, const double *v, const int *cols, long col0,
                              double *Xplus, double *dir) {
  if (k <= 0) return;
  const int wide = (((uintptr_t)Xplus | (uintptr_t)dir) & 15) == 0 ? 1 : 0;
  const long npairs = ((long)(r + 1) * k + 1) / 2;
  hipLaunchKernelGGL(k_lift_images, dim3(vec_grid(npairs)), dim3(kBlock), 0, st, r, k, X, v, cols, col0, Xplus, dir,
                     wide);
}

void launch_lift_images(hipStream_t st, int r, long k, const double *X, const double *v, double *Xplus, double *dir) {
  launch_lift_images_agent(st, r, k, X, v, nullptr, 0, Xplus, dir);
}

}  // namespace dcora
