// What the output frames (output.hip), the zonal means (zonal.hip) and the derived frames (derived.hip) share, stated once: the frame
// definitions, a chunk's neighbours, the under-aligned 4-vector types, the row load and the chunk store.  Device code only; the three
// objects are built STRICT (no contraction, IEEE divide / sqrt), so a statement has the same bits wherever it is inlined.
//
// Placement rule: a binary operation sits at its FIRST operand's location, the second operand is interpolated there, and a divisor
// field is interpolated; all arithmetic in double.  C-grid, cell (i, j); `cons`: the conservative model, which stores uh, vh:
//   U     @fc  q1                      (vector-invariant)    q1 / ℑxᶠh    (conservative)                      frame_vel
//   V     @cf  q2                                            q2 / ℑyᶠh                                        frame_vel
//   SPEED @fc  sqrt(U² + ℑxyᶠᶜ(V²))                                                                           frame_speed
//   BX    @cf  −((A(j) − A(j−1)) / Δy) / ℑyᶠh                                                                 frame_bx
//   BY    @fc   ((A(i) − A(i−1)) / Δx) / ℑxᶠh                                                                 frame_by
//   ℑxyᶠᶜ(g)   0.5*(0.5*(g(i−1,j) + g(i,j)) + 0.5*(g(i−1,j+1) + g(i,j+1)))                                    frame_xy_mean
// spectra_device.inc::frame_value states the same definitions for one cell of one field and must agree with these bit for bit.

constexpr int FRAME_VEC = 4;   // cells of a chunk: 32 B of an fp64 parent, one 16-byte store of a float32 frame

// q at a face between the cells whose depths are ha, hb (in the order of the interpolation's sum)
__device__ __forceinline__ double frame_vel(bool cons, double q, double ha, double hb) { return cons ? q / (0.5 * (ha + hb)) : q; }
// Ac, As: A at the cell and south of it; hs, hc: h south of the face and at it
__device__ __forceinline__ double frame_bx(double Ac, double As, double dy, double hs, double hc) { return -((Ac - As) / dy) / (0.5 * (hs + hc)); }
// Ac, Aw: A at the cell and west of it; hw, hc: h west of the face and at it
__device__ __forceinline__ double frame_by(double Ac, double Aw, double dx, double hw, double hc) { return ((Ac - Aw) / dx) / (0.5 * (hw + hc)); }
// u at the face; g00 g10: V at (i−1, j), (i, j); g01 g11: at (i−1, j+1), (i, j+1)
__device__ __forceinline__ double frame_speed(double u, double g00, double g10, double g01, double g11) {
    return sqrt(u * u + 0.5 * (0.5 * (g00 * g00 + g10 * g10) + 0.5 * (g01 * g01 + g11 * g11)));
}
__device__ __forceinline__ double frame_xy_mean(double a, double b, double c, double d) { return 0.5 * (0.5 * (a + b) + 0.5 * (c + d)); }

// Where the neighbours of the chunk at x0 of row y are: the offsets of rows y, y − 1, y + 1 and the column west of x0.  With wrap bit 0
// (x) / bit 1 (y) they are taken at (x mod Nx, y mod Ny) instead of the halo.
struct FrameRows {
    long r0, rm, rp;
};
__device__ __forceinline__ FrameRows frame_rows(int y, int Ny, long sy, int wrap) {
    const int ym = (y == 0 && (wrap & 2)) ? Ny - 1 : y - 1;
    const int yp = (y == Ny - 1 && (wrap & 2)) ? 0 : y + 1;
    return FrameRows{(long)y * sy, (long)ym * sy, (long)yp * sy};
}
__device__ __forceinline__ int frame_west(int x0, int Nx, int wrap) { return (x0 == 0 && (wrap & 1)) ? Nx - 1 : x0 - 1; }

// Parents and frames are only element-aligned (the interior starts Hx elements into a row; a frame row is Nx elements)
typedef double frame_d4 __attribute__((ext_vector_type(4), aligned(8)));
typedef float frame_f4 __attribute__((ext_vector_type(4), aligned(4)));
template <typename T> struct FrameVec;
template <> struct FrameVec<double> { typedef frame_d4 type; };
template <> struct FrameVec<float> { typedef frame_f4 type; };

// values x0-1, x0 .. x0+3 of one row: r[0] is the west neighbour of the chunk, r[1 + k] cell x0 + k; a chunk that crosses the end of the
// row (!full) is read by single elements.  LEFT: the same index decided by the cells left, Nx - x0, as k_zonal_means' loop decides
// everything (x0 is a multiple of 4 below Nx, so neither form passes 2^31 - 1).  Two texts of one comparison, because each of the two
// kernels compiles to another code object with the other's, and a listing that changes is a change to measure.
template <bool LEFT = false, typename T>
__device__ __forceinline__ void load_row(const T *__restrict__ row, int x0, int xl, bool full, int Nx, double (&r)[FRAME_VEC + 1]) {
    r[0] = (double)row[xl];
    if (full) {
        const typename FrameVec<T>::type v = *reinterpret_cast<const typename FrameVec<T>::type *>(row + x0);
#pragma unroll
        for (int k = 0; k < FRAME_VEC; ++k) r[1 + k] = (double)v[k];
    } else {
#pragma unroll
        for (int k = 0; k < FRAME_VEC; ++k) r[1 + k] = (double)row[(LEFT ? k < Nx - x0 : x0 + k < Nx) ? x0 + k : Nx - 1];   // (beyond the row: never used)
    }
}

template <typename O>
__device__ __forceinline__ void store_chunk(O *__restrict__ p, const double (&v)[FRAME_VEC], bool full, int nvalid) {
    if (full) {
        typename FrameVec<O>::type w;
#pragma unroll
        for (int k = 0; k < FRAME_VEC; ++k) w[k] = (O)v[k];
        *reinterpret_cast<typename FrameVec<O>::type *>(p) = w;
    } else {
#pragma unroll
        for (int k = 0; k < FRAME_VEC; ++k)
            if (k < nvalid) p[k] = (O)v[k];
    }
}
