#include "MathUtilities.h"

// Reverse-Z puts far at 0 and near at 1; the infinite variant drops the far plane
// (reference source/MathUtilities.cpp:3-38: only _33 and _43 change).
void ModifyPerspectiveMatrix(Matrix& mat, float nearPlane, float farPlane, bool bReverseZ, bool bInfiniteZ)
{
    float q1 = 0.0f, q2 = 0.0f;
    if (bReverseZ) {
        q1 = bInfiniteZ ? 0.0f : nearPlane / (farPlane - nearPlane);
        q2 = bInfiniteZ ? nearPlane : q1 * farPlane;
    } else {
        q1 = bInfiniteZ ? -1.0f : farPlane / (nearPlane - farPlane);
        q2 = bInfiniteZ ? -nearPlane : q1 * nearPlane;
    }
    mat.m[2][2] = q1;
    mat.m[3][2] = q2;
}

Matrix CreatePerspectiveFieldOfView(float fovY, float aspect, float nearPlane, float farPlane)
{
    const float h = 1.0f / std::tan(0.5f * fovY);
    const float w = h / aspect;
    const float range = farPlane / (nearPlane - farPlane);
    Matrix p{};
    p.m[0][0] = w;
    p.m[1][1] = h;
    p.m[2][2] = range;
    p.m[2][3] = -1.0f;
    p.m[3][2] = range * nearPlane;
    return p;
}

// See MathUtilities.h.  The operation order is part of the definition (toyrenderer_amd/interop.py clip_to_world repeats it, so that
// both host sides hand the GPU the same 16 numbers): the product's elements summed left to right; a cofactor is +-1 times the 3x3
// determinant a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20) of the minor, summed
// left to right; the determinant expands along row 0, summed left to right; inverse[j][i] = cofactor[i][j] / determinant + 0.0
// (the sum turns a -0 into +0).  A camera's structural zeros (three elements of the last column) come out as exact zeros.
Matrix InverseOfProduct(const Matrix& a, const Matrix& b)
{
    double m[4][4], cof[4][4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            m[i][j] = (((double)a.m[i][0] * (double)b.m[0][j] + (double)a.m[i][1] * (double)b.m[1][j]) + (double)a.m[i][2] * (double)b.m[2][j]) + (double)a.m[i][3] * (double)b.m[3][j];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            int r[3], c[3];
            for (int k = 0, n = 0; k < 4; ++k) if (k != i) r[n++] = k;
            for (int k = 0, n = 0; k < 4; ++k) if (k != j) c[n++] = k;
            auto e = [&](int y, int x) { return m[r[y]][c[x]]; };
            const double d = (e(0, 0) * (e(1, 1) * e(2, 2) - e(1, 2) * e(2, 1)) - e(0, 1) * (e(1, 0) * e(2, 2) - e(1, 2) * e(2, 0))) + e(0, 2) * (e(1, 0) * e(2, 1) - e(1, 1) * e(2, 0));
            cof[i][j] = ((i + j) & 1) ? -d : d;
        }
    const double det = ((m[0][0] * cof[0][0] + m[0][1] * cof[0][1]) + m[0][2] * cof[0][2]) + m[0][3] * cof[0][3];
    Matrix inv;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) inv.m[j][i] = (float)(cof[i][j] / det + 0.0);
    return inv;
}
