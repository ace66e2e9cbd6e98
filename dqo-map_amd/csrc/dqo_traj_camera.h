// The camera of a world pose, in double, for the kernels that form one: traj_append_kernel (map_traj.hip) and traj_repose_kernel
// (map_repose.hip).  Camera.updatePose / update (scene/cameras.py:165-183) with one rounding per statement, none contracted; both files
// are compiled with -ffp-contract=off and tests/traj_oracle.py restates the statements in this order:
//     w2c          the inverse of the AFFINE pose by the cofactors of its 3x3 block R (cameras.py:166 calls np.linalg.inv, and R is
//                  orthonormal only to float32, so not the transpose):
//                      c00 = r11 r22 - r12 r21   c01 = r12 r20 - r10 r22   c02 = r10 r21 - r11 r20
//                      c10 = r02 r21 - r01 r22   c11 = r00 r22 - r02 r20   c12 = r01 r20 - r00 r21
//                      c20 = r01 r12 - r02 r11   c21 = r02 r10 - r00 r12   c22 = r00 r11 - r01 r10
//                      det = (r00 c00 + r01 c01) + r02 c02;   W[a][b] = c[b][a] / det;   T[a] = -((W[a][0] t0 + W[a][1] t1) + W[a][2] t2)
//     camera       c2w = float(pose); w2c = float([W T; 0 0 0 1]) row-major; viewmatrix = float(w2c transposed) (cameras.py:174-178);
//                  projmatrix = float(w2c transposed @ double(projection)), entry = ((a0 b0 + a1 b1) + a2 b2) + a3 b3 in double, rounded
//                  once (:179-183 form the product in float32 from the rounded viewmatrix, which lands up to 1.25 ulp from the double
//                  product; this is within half an ulp of it); campos = float(the pose's translation)
// Every destination is written with 4-byte stores and may be NULL (that one is skipped); nothing outside its extent is written.
#ifndef DQO_TRAJ_CAMERA_H_
#define DQO_TRAJ_CAMERA_H_

// w2c (W 3x3 row-major, T 3) of the affine pose P (4x4 row-major) by the cofactors of its 3x3 block (the head comment's statements)
__device__ __forceinline__ void traj_invert_affine(const double* P, double* W, double* T) {
#pragma clang fp contract(off)
    const double r00 = P[0], r01 = P[1], r02 = P[2], r10 = P[4], r11 = P[5], r12 = P[6], r20 = P[8], r21 = P[9], r22 = P[10];
    const double c00 = r11 * r22 - r12 * r21, c01 = r12 * r20 - r10 * r22, c02 = r10 * r21 - r11 * r20;
    const double c10 = r02 * r21 - r01 * r22, c11 = r00 * r22 - r02 * r20, c12 = r01 * r20 - r00 * r21;
    const double c20 = r01 * r12 - r02 * r11, c21 = r02 * r10 - r00 * r12, c22 = r00 * r11 - r01 * r10;
    const double det = (r00 * c00 + r01 * c01) + r02 * c02;
    W[0] = c00 / det, W[1] = c10 / det, W[2] = c20 / det;
    W[3] = c01 / det, W[4] = c11 / det, W[5] = c21 / det;
    W[6] = c02 / det, W[7] = c12 / det, W[8] = c22 / det;
    const double t0 = P[3], t1 = P[7], t2 = P[11];
    for (int a = 0; a < 3; a++) T[a] = -((W[3 * a] * t0 + W[3 * a + 1] * t1) + W[3 * a + 2] * t2);
}

// The camera tensors of the pose P whose inverse is (W, T); projection (float32 [16], transposed as the reference keeps it) is read only
// for projmatrix and must be there when projmatrix is.
__device__ __forceinline__ void traj_store_camera(const double* P, const double* W, const double* T, const float* __restrict__ projection,
                                                  float* __restrict__ c2w, float* __restrict__ w2c, float* __restrict__ viewmatrix,
                                                  float* __restrict__ projmatrix, float* __restrict__ campos) {
#pragma clang fp contract(off)
    if (c2w)
        for (int k = 0; k < 16; k++) c2w[k] = (float)P[k];
    if (campos) campos[0] = (float)P[3], campos[1] = (float)P[7], campos[2] = (float)P[11];
    if (w2c) {
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) w2c[4 * a + b] = (float)W[3 * a + b];
            w2c[4 * a + 3] = (float)T[a];
            w2c[12 + a] = 0.0f;
        }
        w2c[15] = 1.0f;
    }
    if (viewmatrix || projmatrix) {
        double V[16];  // w2c transposed: the reference's world_view_transform, still in double
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) V[4 * b + a] = W[3 * a + b];
            V[12 + a] = T[a];
            V[4 * a + 3] = 0.0;
        }
        V[15] = 1.0;
        if (viewmatrix)
            for (int k = 0; k < 16; k++) viewmatrix[k] = (float)V[k];
        if (projmatrix) {
            double Q[16];
            for (int k = 0; k < 16; k++) Q[k] = (double)projection[k];
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++)
                    projmatrix[4 * r + c] =
                        (float)(((V[4 * r] * Q[c] + V[4 * r + 1] * Q[4 + c]) + V[4 * r + 2] * Q[8 + c]) + V[4 * r + 3] * Q[12 + c]);
        }
    }
}

#endif  // DQO_TRAJ_CAMERA_H_
