/* gcge_pas.h — the composite (augmented) operator table of the PAS eigensolver.
 *
 * PAS (parallel augmented subspace, the reference's src/ops_eig_sol_pas.c with app/app_pas.c) solves the Rayleigh-Ritz
 * problem of the fine level on the augmented space  span{ P_H (all coarse functions) } + span{ X (s fine vectors) }.  In
 * that basis the projected pencil is
 *     A = [[ A_H , QX ], [ QX^T , XX ]]        B = [[ B_H , 0 ], [ 0 , I ]]
 * with A_H the Galerkin coarse matrix, QX (n_H x s) the restriction of A X to level H, XX = X^T A X (s x s, host) and
 * X B-orthonormal and B-orthogonal to range(P_H).  OPS_PAS_Set fills a table whose matrices are PASMAT and whose blocks
 * of vectors are PASVEC; every slot works through the app_ops slots on the coarse part plus host dense work on the tail,
 * so the same code runs over every back-end.  Inner products add the tail after the coarse part has been reduced over
 * the ranks (the tail is replicated: it counts once).
 */
#ifndef GCGE_PAS_H
#define GCGE_PAS_H

#include "gcge_ops.h"

#ifdef __cplusplus
extern "C" {
#endif

/* [[alpha QQ, QX], [QX^T, XX]]; QX == NULL: [[alpha QQ, 0], [0, I]] (the B of the pencil) */
typedef struct PASMAT_ {
	void   *QQ;        /* coarse matrix of app_ops (A_H or B_H)                                              */
	double  alpha;     /* its factor: scale^-H for the scaled A_H of our hierarchies (a power of two), 1 else */
	void  **QX;        /* n_H x size block of app_ops (columns 0 .. size), NULL: the border is zero          */
	double *XX;        /* size x size host, column-major, leading dimension size; NULL: identity             */
	int     size;      /* s, the rows of the tail                                                            */
	void   *mat_H;     /* the matrix MultiVecCreateByMat of app_ops is given for the coarse parts (A_H)      */
} PASMAT;

/* coarse part q (ncols columns of app_ops) + tail x (size x ncols, host, column-major: a GCGE_DENSE) */
typedef struct PASVEC_ {
	void      **q;
	GCGE_DENSE  x;
	int         owned;  /* 1: created by the table's slots (destroyed with it); 0: a wrapper around caller blocks */
} PASVEC;

void OPS_PAS_Set (struct OPS_ *pas_ops, struct OPS_ *app_ops);

/* The fused bordered product of a back-end (GCGE_BACKEND.pas_border): with QX the first s columns of the row blocks `QX`,
 *     y[:, y0 .. y0 + m) = beta y[:, y0 .. y0 + m) + QX t        g = QX^T q[:, q0 .. q0 + m)   (LOCAL rows only)
 * t (s x m, ld ldt) and g (s x m, ld ldg) in host memory.  Returns 0, nonzero: declined (the caller uses the slots).      */
typedef int (*GCGE_PAS_BORDER_FN) (void **QX, int s, void **q, int q0, void **y, int y0, int m, double beta,
		const double *t, int ldt, double *g, int ldg);

/* The identity of a standard problem (B == NULL), uploaded once at set-up: the hierarchy built from it holds the coarse masses
 * P^T P (diagonal: the aggregate sizes).  The back-end's record offers it (GCGE_BACKEND.mat_identity / mat_free); a table
 * without a record may register its own here (NULL clears).  GCGE_PAS_MatIdentityOf: what applies to `ops` (NULL: none). */
typedef void *(*GCGE_MAT_IDENTITY_FN) (void *like);
typedef void  (*GCGE_MAT_FREE_FN) (void *mat);
void GCGE_PAS_SetMatIdentity (GCGE_MAT_IDENTITY_FN identity, GCGE_MAT_FREE_FN mat_free);
GCGE_MAT_IDENTITY_FN GCGE_PAS_MatIdentityOf (struct OPS_ *ops, GCGE_MAT_FREE_FN *mat_free);

#ifdef __cplusplus
}
#endif
#endif
