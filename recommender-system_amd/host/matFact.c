/*
 * matFact.c -- the drop-in command line: `matFact <file.in>` with the reference's argv handling, input
 * grammar, stdout format and error convention (matFact.c:61-137, util.c:7-10), the iteration loop and the
 * recommendation step running on an MI355X through the C ABI of include/matfact_hip.h.
 *
 * stdout carries ONLY the recommendations (one index per line), byte-identical to the reference's `.out`
 * files; timing goes to stderr and only when MATFACT_TIMING is set (the root-dir reference build appends a
 * `time : %f` line to stdout, benchmark.h:23; the hand-in build prints none).
 */
#define _POSIX_C_SOURCE 200809L
#include "../../include/matfact_hip.h"
#include "../../include/matfact_host.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

/*
 * MATFACT_MATS=<path>: also write the reference's debug dump format (samples/inst{0,1,2}.mats): the dense
 * rating matrix, then L, R (printed K x I, i.e. un-transposed) and B = L R^T with "%f " per element -- initially,
 * after each of the first MATFACT_MATS_ITERS iterations (default 0; inst0.mats holds 5) and at the end.
 * Uses the resident-plan API so that every number printed comes from the GPU path.
 */
static void mats_matrix(FILE *f, const char *title, const double *m, int rows, int cols, int transposed)
{
	fprintf(f, "%s\n", title);
	for (int i = 0; i < rows; i++) {
		for (int j = 0; j < cols; j++)
			fprintf(f, "%f ", transposed ? m[(size_t) j * rows + i] : m[(size_t) i * cols + j]);
		fprintf(f, "\n");
	}
}

static int mats_state(FILE *f, mf_plan *plan, const mf_problem *p, double *L, double *R, double *B, int initial)
{
	int rc = mf_plan_download_factors(plan, L, R);
	if (rc == MF_OK) rc = mf_plan_predict(plan, B);
	if (rc != MF_OK) return rc;
	mats_matrix(f, initial ? "Initial matrix L" : "Matrix L", L, p->users, p->features, 0);
	mats_matrix(f, initial ? "Initial matrix R" : "Matrix R", R, p->features, p->items, 1);
	mats_matrix(f, initial ? "Initial matrix B" : "Matrix B", B, p->users, p->items, 0);
	return MF_OK;
}

static int run_with_mats(const char *path, const mf_problem *p, double *L, double *R, int32_t *best, int device)
{
	/* the dense A and B of the dump exist only for small instances (mf_plan_predict refuses more than 2^26 elements);
	 * indices are checked BEFORE A is filled: the parser does not range-check them, only the device build does */
	const size_t nb = (size_t) p->users * (size_t) p->items;
	if (p->users < 0 || p->items < 0 || nb > ((size_t) 1 << 26)) return MF_ERR_UNSUPPORTED;
	for (int64_t n = 0; n < p->nnz; n++)
		if (p->entries[n].row < 0 || p->entries[n].row >= p->users || p->entries[n].col < 0 ||
		    p->entries[n].col >= p->items)
			return MF_ERR_ARGUMENT;
	int rc = MF_OK;
	FILE *f = fopen(path, "w");
	double *B = calloc(nb ? nb : 1, sizeof(double));
	int32_t *row = malloc(sizeof(int32_t) * (size_t) (p->nnz ? p->nnz : 1));
	int32_t *col = malloc(sizeof(int32_t) * (size_t) (p->nnz ? p->nnz : 1));
	double *val = malloc(sizeof(double) * (size_t) (p->nnz ? p->nnz : 1));
	mf_plan *plan = NULL;
	if (!f) rc = MF_ERR_ARGUMENT;
	if (rc == MF_OK && (!B || !row || !col || !val)) rc = MF_ERR_NO_MEMORY;
	if (rc != MF_OK) goto done;
	mf_host_split_entries(p->entries, p->nnz, row, col, val);
	for (int64_t n = 0; n < p->nnz; n++) B[(size_t) row[n] * p->items + col[n]] = val[n];
	mats_matrix(f, "Initial matrix A", B, p->users, p->items, 0);

	mf_shard s = {p->users, p->items, p->features, 0, p->users, p->nnz, row, col, val, p->alpha, device, 0, {0, 0}, {0, 0}, 0, 0};
	rc = mf_plan_create(&plan, &s);
	if (rc == MF_OK) rc = mf_plan_upload_factors(plan, L, R);
	if (rc == MF_OK) rc = mats_state(f, plan, p, L, R, B, 1);
	int shown = getenv("MATFACT_MATS_ITERS") ? atoi(getenv("MATFACT_MATS_ITERS")) : 0;
	if (shown > p->iters) shown = p->iters;
	for (int it = 0; rc == MF_OK && it < shown; it++) {
		rc = mf_plan_iterate(plan, 1);
		if (rc == MF_OK) {
			fprintf(f, "Iter=%d\n", it);
			rc = mats_state(f, plan, p, L, R, B, 0);
		}
	}
	if (rc == MF_OK) rc = mf_plan_iterate(plan, p->iters - shown);
	if (rc == MF_OK) {
		fprintf(f, "Final:\n");
		rc = mats_state(f, plan, p, L, R, B, 0);
	}
	if (rc == MF_OK) rc = mf_plan_recommend(plan, best);
done:   /* the one way out: everything that was acquired is released, whatever failed */
	mf_plan_destroy(plan);
	free(B);
	free(row);
	free(col);
	free(val);
	if (f && fclose(f) == EOF && rc == MF_OK) rc = MF_ERR_ARGUMENT;
	return rc;
}

/*
 * MATFACT_CHECKPOINT=<path> [MATFACT_CHECKPOINT_EVERY=n, default 1000]: write (L, R, iterations done) every n
 * iterations; MATFACT_RESUME=<path>: start from such a file instead of the random initial factors.  The final
 * factors and recommendations are bit-identical to an uninterrupted run.
 */
static int run_with_checkpoints(const mf_problem *p, double *L, double *R, int32_t *best, int device, int start_iter)
{
	const char *ck = getenv("MATFACT_CHECKPOINT");
	int every = getenv("MATFACT_CHECKPOINT_EVERY") ? atoi(getenv("MATFACT_CHECKPOINT_EVERY")) : 1000;
	if (every < 1) every = 1;
	int32_t *row = malloc(sizeof(int32_t) * (size_t) (p->nnz ? p->nnz : 1));
	int32_t *col = malloc(sizeof(int32_t) * (size_t) (p->nnz ? p->nnz : 1));
	double *val = malloc(sizeof(double) * (size_t) (p->nnz ? p->nnz : 1));
	if (!row || !col || !val) return MF_ERR_NO_MEMORY;
	mf_host_split_entries(p->entries, p->nnz, row, col, val);
	mf_shard s = {p->users, p->items, p->features, 0, p->users, p->nnz, row, col, val, p->alpha, device, 0, {0, 0}, {0, 0}, 0, 0};
	mf_plan *plan = NULL;
	int rc = mf_plan_create(&plan, &s);
	if (rc == MF_OK) rc = mf_plan_upload_factors(plan, L, R);
	int done = start_iter;
	while (rc == MF_OK && done < p->iters) {
		int step = p->iters - done;
		if (ck && step > every - done % every) step = every - done % every;
		rc = mf_plan_iterate(plan, step);
		done += step;
		if (rc == MF_OK && ck && done < p->iters) {
			rc = mf_plan_download_factors(plan, L, R);
			if (rc == MF_OK && mf_host_checkpoint_write(ck, p, done, L, R) != 0) rc = MF_ERR_ARGUMENT;
		}
	}
	if (rc == MF_OK) rc = mf_plan_recommend(plan, best);
	if (rc == MF_OK) rc = mf_plan_download_factors(plan, L, R);
	mf_plan_destroy(plan);
	free(row);
	free(col);
	free(val);
	return rc;
}

/*
 * MATFACT_LOSS=every[,tol] [MATFACT_HELDOUT=<file.in>]: the single-GPU run through mf_plan_iterate_monitored.  One line per
 * evaluated point goes to stderr; stdout is the `.out` of the iterations actually run (all of them when tol is absent).
 * With MATFACT_LAMBDA the loop runs regularised, and one more stderr line after it carries ||L||^2, ||R||^2
 * (mf_plan_penalty) and the objective SSE + lambda_users ||L||^2 + lambda_items ||R||^2 of the final factors.
 * With MATFACT_BIAS (`biased`) the caller hands in the packed problem of K = F + 2 -- values centred with the training mean
 * `mu`, the held-out ones too, factors packed by mf_backend_bias_pack --, the loop runs with the users' column K-1 and the
 * items' column K-2 frozen, and one more stderr line behind the points carries mu.
 */
static int run_with_loss(const mf_problem *p, const mf_problem *held, const double *L, const double *R, int32_t *best, int device,
                         int every, double tol, int rank_cutoff, int regularised, double lambda_users, double lambda_items, int biased, double mu)
{
	const int64_t nmax = p->nnz > (held ? held->nnz : 0) ? p->nnz : (held ? held->nnz : 0);
	int32_t *row = malloc(sizeof(int32_t) * (size_t) (nmax ? nmax : 1));
	int32_t *col = malloc(sizeof(int32_t) * (size_t) (nmax ? nmax : 1));
	double *val = malloc(sizeof(double) * (size_t) (nmax ? nmax : 1));
	const int cap = p->iters / every + 2;
	mf_loss_point *trace = malloc(sizeof(mf_loss_point) * (size_t) cap);
	if (!row || !col || !val || !trace) return MF_ERR_NO_MEMORY;
	mf_host_split_entries(p->entries, p->nnz, row, col, val);
	mf_shard s = {p->users, p->items, p->features, 0, p->users, p->nnz, row, col, val, p->alpha, device, 0, {0, 0}, {0, 0}, 0, 0};
	mf_plan *plan = NULL;
	int rc = mf_plan_create(&plan, &s);
	if (rc == MF_OK) rc = mf_plan_upload_factors(plan, L, R);
	if (rc == MF_OK && held) {
		mf_host_split_entries(held->entries, held->nnz, row, col, val);
		rc = mf_plan_set_heldout(plan, held->nnz, row, col, val);
	}
	int points = 0, done = 0;
	if (rc == MF_OK && regularised) rc = mf_plan_set_regularization(plan, lambda_users, lambda_items);
	if (rc == MF_OK && biased) rc = mf_plan_set_frozen_columns(plan, p->features - 1, p->features - 2);
	if (rc == MF_OK) rc = mf_plan_iterate_monitored(plan, p->iters, every, tol, trace, cap, &points, &done);
	for (int i = 0; rc == MF_OK && i < points && i < cap; i++) {
		fprintf(stderr, "iter %d train_rmse %.17g", trace[i].iter,
		        trace[i].train.count > 0 ? sqrt(trace[i].train.sse / (double) trace[i].train.count) : NAN);
		if (held && held->nnz > 0)
			fprintf(stderr, " heldout_rmse %.17g", sqrt(trace[i].heldout.sse / (double) trace[i].heldout.count));
		fprintf(stderr, "\n");
	}
	if (rc == MF_OK && biased) fprintf(stderr, "bias mu %.17g\n", mu);
	if (rc == MF_OK && regularised) {
		/* MATFACT_LAMBDA: the penalty's norms of the final factors and the objective at them */
		double lsq = 0.0, rsq = 0.0;
		mf_loss fin;
		rc = mf_plan_penalty(plan, &lsq, &rsq, NULL, NULL);
		if (rc == MF_OK) rc = mf_plan_loss(plan, MF_LOSS_TRAIN, &fin, NULL);
		if (rc == MF_OK)
			fprintf(stderr, "penalty lambda %.17g %.17g users_sq %.17g items_sq %.17g objective %.17g\n", lambda_users, lambda_items, lsq,
			        rsq, (fin.sse + lambda_users * lsq) + lambda_items * rsq);
	}
	if (rc == MF_OK && rank_cutoff && held && held->nnz > 0) {
		/* row still holds the users of the held-out entries in the caller's order; col is free to take the ranks */
		rc = mf_plan_rank_heldout(plan, col);
		mf_rank_metrics m;
		if (rc == MF_OK) rc = mf_backend_rank_metrics(col, row, held->nnz, rank_cutoff, &m);
		if (rc == MF_OK)
			fprintf(stderr, "heldout_rank cutoff %d evaluated %lld masked %lld nan %lld users %lld hits %lld hit_rate %.17g mrr %.17g ndcg %.17g\n",
			        rank_cutoff, (long long) m.evaluated, (long long) m.masked, (long long) m.nan, (long long) m.users,
			        (long long) m.hits, m.hit_rate, m.mrr, m.ndcg);
	} else if (rc == MF_OK && rank_cutoff) {
		fprintf(stderr, "heldout_rank cutoff %d evaluated 0 masked 0 nan 0 users 0 hits 0 hit_rate %.17g mrr %.17g ndcg %.17g\n", rank_cutoff,
		        NAN, NAN, NAN);
	}
	if (rc == MF_OK) rc = mf_plan_recommend(plan, best);
	mf_plan_destroy(plan);
	free(row);
	free(col);
	free(val);
	free(trace);
	return rc;
}

/*
 * MATFACT_SIMILAR=N[,dot|cosine] MATFACT_SIMILAR_OUT=<path>: after training, the N nearest other items of every item by
 * that metric (mf_plan_similar_items on the trained R) go to <path>, one line per item in mf_host_write_topn's format;
 * stdout is the usual `.out`.
 */
static int run_with_similar(const mf_problem *p, const double *L, const double *R, int32_t *best, int device, int n, int metric,
                            const char *out_path)
{
	int32_t *row = malloc(sizeof(int32_t) * (size_t) (p->nnz ? p->nnz : 1));
	int32_t *col = malloc(sizeof(int32_t) * (size_t) (p->nnz ? p->nnz : 1));
	double *val = malloc(sizeof(double) * (size_t) (p->nnz ? p->nnz : 1));
	int32_t *near = malloc(sizeof(int32_t) * (size_t) (p->items > 0 ? p->items : 1) * (size_t) n);
	mf_plan *plan = NULL;
	int rc = row && col && val && near ? MF_OK : MF_ERR_NO_MEMORY;
	if (rc == MF_OK) {
		mf_host_split_entries(p->entries, p->nnz, row, col, val);
		mf_shard s = {p->users, p->items, p->features, 0, p->users, p->nnz, row, col, val, p->alpha, device, 0, {0, 0}, {0, 0}, 0, 0};
		rc = mf_plan_create(&plan, &s);
	}
	if (rc == MF_OK) rc = mf_plan_upload_factors(plan, L, R);
	if (rc == MF_OK) rc = mf_plan_iterate(plan, p->iters);
	if (rc == MF_OK) rc = mf_plan_recommend(plan, best);
	if (rc == MF_OK) rc = mf_plan_similar_items(plan, metric, NULL, p->items, n, near, NULL);
	if (rc == MF_OK) {
		FILE *f = fopen(out_path, "w");
		if (!f || mf_host_write_topn(f, near, p->items, n) != 0) rc = MF_ERR_ARGUMENT;
		if (f && fclose(f) == EOF) rc = MF_ERR_ARGUMENT;
	}
	mf_plan_destroy(plan);
	free(row);
	free(col);
	free(val);
	free(near);
	return rc;
}

/* util.c:7-10 */
static void die(const char *error)
{
	fprintf(stderr, "Error: %s\n", error);
	exit(-1);
}

/* MATFACT_BIAS: a copy of `p` with K = F + 2 and every value centred with `mu` (one rounding each); NULL when out of memory */
static mf_entry *centred_entries(const mf_problem *p, double mu)
{
	mf_entry *e = malloc(sizeof(mf_entry) * (size_t) (p->nnz ? p->nnz : 1));
	for (int64_t n = 0; e && n < p->nnz; n++) {
		e[n] = p->entries[n];
		e[n].value = p->entries[n].value - mu;
	}
	return e;
}

/*
 * MATFACT_BIAS=1 with MATFACT_LOSS: the monitored loop on the packed plan.  L and R hold the reference's initialisation for
 * K = F; the biases start at 0.0; the held-out values are centred with the TRAINING mean.
 */
static int run_biased_with_loss(const mf_problem *p, const mf_problem *held, const double *L, const double *R, int32_t *best, int device,
                                int every, double tol, int rank_cutoff, int regularised, double lambda_users, double lambda_items)
{
	const int32_t F = p->features, K = F + 2;
	double mu = 0.0;
	double *val = malloc(sizeof(double) * (size_t) (p->nnz ? p->nnz : 1));
	double *Lp = malloc(sizeof(double) * ((size_t) p->users * (size_t) K + 1));
	double *Rp = malloc(sizeof(double) * ((size_t) p->items * (size_t) K + 1));
	if (!val || !Lp || !Rp) return MF_ERR_NO_MEMORY;
	for (int64_t n = 0; n < p->nnz; n++) val[n] = p->entries[n].value;
	int rc = mf_backend_bias_mean(val, p->nnz, &mu);
	free(val);
	mf_problem q = *p, h;
	q.features = K;
	mf_entry *qe = centred_entries(p, mu), *he = NULL;
	q.entries = qe;
	if (held) {
		h = *held;
		h.features = K;
		he = centred_entries(held, mu);
		h.entries = he;
	}
	if (!qe || (held && !he)) rc = MF_ERR_NO_MEMORY;
	if (rc == MF_OK) rc = mf_backend_bias_pack(L, NULL, p->users, F, 1, Lp);
	if (rc == MF_OK) rc = mf_backend_bias_pack(R, NULL, p->items, F, 0, Rp);
	if (rc == MF_OK)
		rc = run_with_loss(&q, held ? &h : NULL, Lp, Rp, best, device, every, tol, rank_cutoff, regularised, lambda_users, lambda_items, 1, mu);
	free(qe);
	free(he);
	free(Lp);
	free(Rp);
	return rc;
}

static double now(void)
{
	struct timespec t;
	clock_gettime(CLOCK_MONOTONIC, &t);
	return (double) t.tv_sec + 1e-9 * (double) t.tv_nsec;
}

int main(int argc, char **argv)
{
	if (argc != 2) {
		fprintf(stderr, "Run ./matFact.out file");   /* matFact.c:65 */
		die("Missing input file name.");
	}
	/* MATFACT_TOPN=N (1..MF_TOPN_MAX): N items per user on one line each instead of one (mf_host_write_topn); the single-GPU
	 * default path only.  Checked before the input is read: a bad value prints nothing. */
	int topn = 0;
	const char *topn_env = getenv("MATFACT_TOPN");
	if (topn_env) {
		char *stop;
		const long v = strtol(topn_env, &stop, 10);
		if (stop == topn_env || *stop || v < 1 || v > MF_TOPN_MAX) die("MATFACT_TOPN: expected a whole number from 1 to 32.");
		if (getenv("MATFACT_DEVICES") || getenv("MATFACT_MATS") || getenv("MATFACT_CHECKPOINT") || getenv("MATFACT_RESUME"))
			die("MATFACT_TOPN works on the single-GPU path only: unset MATFACT_DEVICES, MATFACT_MATS, MATFACT_CHECKPOINT and MATFACT_RESUME.");
		topn = (int) v;
	}
	/* MATFACT_LOSS=every[,tol]: training (and, with MATFACT_HELDOUT=<file.in>, held-out) RMSE every `every` iterations on
	 * stderr; with tol the run stops by the rule of mf_plan_iterate_monitored.  The single-GPU default path only. */
	int loss_every = 0;
	double loss_tol = 0.0;
	const char *loss_env = getenv("MATFACT_LOSS");
	if (loss_env) {
		char *stop;
		const long v = strtol(loss_env, &stop, 10);
		if (stop == loss_env || v < 1 || v > 2147483647L || (*stop && *stop != ',')) die("MATFACT_LOSS: expected every[,tol] with every a whole number >= 1.");
		if (*stop == ',') {
			char *stop2;
			loss_tol = strtod(stop + 1, &stop2);
			if (stop2 == stop + 1 || *stop2) die("MATFACT_LOSS: expected every[,tol] with tol a number.");
		}
		if (getenv("MATFACT_DEVICES") || getenv("MATFACT_MATS") || getenv("MATFACT_CHECKPOINT") || getenv("MATFACT_RESUME") || topn)
			die("MATFACT_LOSS works on the single-GPU path only: unset MATFACT_DEVICES, MATFACT_MATS, MATFACT_CHECKPOINT, MATFACT_RESUME and MATFACT_TOPN.");
		loss_every = (int) v;
	} else if (getenv("MATFACT_HELDOUT"))
		die("MATFACT_HELDOUT needs MATFACT_LOSS=every[,tol].");
	/* MATFACT_RANK=N (N >= 1) with MATFACT_LOSS and MATFACT_HELDOUT: after the monitored loop one more stderr line with the
	 * hit rate, MRR and NDCG at N of the held-out entries' ranks (mf_plan_rank_heldout, mf_backend_rank_metrics) */
	int rank_cutoff = 0;
	const char *rank_env = getenv("MATFACT_RANK");
	if (rank_env) {
		char *stop;
		const long v = strtol(rank_env, &stop, 10);
		if (stop == rank_env || *stop || v < 1 || v > 2147483647L) die("MATFACT_RANK: expected a whole number >= 1.");
		if (!loss_every || !getenv("MATFACT_HELDOUT")) die("MATFACT_RANK needs MATFACT_HELDOUT=<file.in>.");
		rank_cutoff = (int) v;
	}
	/* MATFACT_SIMILAR=N[,dot|cosine] (1..MF_TOPN_MAX, default cosine) with MATFACT_SIMILAR_OUT=<path>: the N nearest other
	 * items of every item, one line per item, to <path>; stdout is unchanged.  The single-GPU default path only. */
	int similar = 0, similar_metric = MF_SIMILAR_COSINE;
	const char *similar_env = getenv("MATFACT_SIMILAR");
	if (similar_env) {
		char *stop;
		const long v = strtol(similar_env, &stop, 10);
		if (stop == similar_env || v < 1 || v > MF_TOPN_MAX || (*stop && *stop != ','))
			die("MATFACT_SIMILAR: expected N[,dot|cosine] with N a whole number from 1 to 32.");
		if (*stop == ',') {
			if (!strcmp(stop + 1, "dot")) similar_metric = MF_SIMILAR_DOT;
			else if (strcmp(stop + 1, "cosine")) die("MATFACT_SIMILAR: expected N[,dot|cosine] with N a whole number from 1 to 32.");
		}
		if (!getenv("MATFACT_SIMILAR_OUT") || !*getenv("MATFACT_SIMILAR_OUT")) die("MATFACT_SIMILAR needs MATFACT_SIMILAR_OUT=<path>.");
		if (getenv("MATFACT_DEVICES") || getenv("MATFACT_MATS") || getenv("MATFACT_CHECKPOINT") || getenv("MATFACT_RESUME"))
			die("MATFACT_SIMILAR works on the single-GPU path only: unset MATFACT_DEVICES, MATFACT_MATS, MATFACT_CHECKPOINT and MATFACT_RESUME.");
		if (topn || loss_every) die("MATFACT_SIMILAR cannot be combined with MATFACT_TOPN or MATFACT_LOSS.");
		similar = (int) v;
	} else if (getenv("MATFACT_SIMILAR_OUT"))
		die("MATFACT_SIMILAR_OUT needs MATFACT_SIMILAR=N[,dot|cosine].");
	/* MATFACT_LAMBDA=l[,li]: L2 regularisation, one number for both sides or users,items (mf_plan_set_regularization's
	 * rule: finite and >= 0).  The single-GPU default path (mf_backend_run_reg) and the MATFACT_LOSS path only. */
	int regularised = 0;
	double lambda_users = 0.0, lambda_items = 0.0;
	const char *lambda_env = getenv("MATFACT_LAMBDA");
	if (lambda_env) {
		char *stop;
		lambda_users = lambda_items = strtod(lambda_env, &stop);
		if (stop == lambda_env || (*stop && *stop != ',')) die("MATFACT_LAMBDA: expected l[,li] with l and li numbers >= 0.");
		if (*stop == ',') {
			char *stop2;
			lambda_items = strtod(stop + 1, &stop2);
			if (stop2 == stop + 1 || *stop2) die("MATFACT_LAMBDA: expected l[,li] with l and li numbers >= 0.");
		}
		if (!isfinite(lambda_users) || !isfinite(lambda_items) || lambda_users < 0.0 || lambda_items < 0.0)
			die("MATFACT_LAMBDA: expected l[,li] with l and li numbers >= 0.");
		if (getenv("MATFACT_DEVICES") || getenv("MATFACT_MATS") || getenv("MATFACT_CHECKPOINT") || getenv("MATFACT_RESUME") || topn || similar)
			die("MATFACT_LAMBDA works on the single-GPU path only: unset MATFACT_DEVICES, MATFACT_MATS, MATFACT_CHECKPOINT, MATFACT_RESUME, MATFACT_TOPN and MATFACT_SIMILAR.");
		regularised = 1;
	}
	/* MATFACT_BIAS=1: the biased model a ~ mu + b_user + b_item + l.r on frozen columns (mf_backend_run_biased); the file's K
	 * is the latent count F.  The single-GPU default path and the MATFACT_LOSS path only, with or without MATFACT_LAMBDA. */
	int biased = 0;
	const char *bias_env = getenv("MATFACT_BIAS");
	if (bias_env) {
		if (strcmp(bias_env, "1")) die("MATFACT_BIAS: expected 1.");
		if (getenv("MATFACT_DEVICES") || getenv("MATFACT_MATS") || getenv("MATFACT_CHECKPOINT") || getenv("MATFACT_RESUME") || topn || similar)
			die("MATFACT_BIAS works on the single-GPU path only: unset MATFACT_DEVICES, MATFACT_MATS, MATFACT_CHECKPOINT, MATFACT_RESUME, MATFACT_TOPN and MATFACT_SIMILAR.");
		biased = 1;
	}
	const double t0 = now();

	mf_problem prob;
	/* MATFACT_CACHE=<dir>: binary cache of parsed inputs keyed by the file's content (util.c:30-34 re-parses every
	 * run); unset: the plain parser */
	int cache_hit = 0;
	const int prc = mf_host_parse_file_cached(argv[1], getenv("MATFACT_CACHE"), &prob, &cache_hit);
	if (prc != MF_PARSE_OK) die(mf_host_parse_strerror(prc));
	mf_problem held;
	const int have_held = loss_every && getenv("MATFACT_HELDOUT");
	if (have_held) {
		const int hrc = mf_host_parse_file(getenv("MATFACT_HELDOUT"), &held);
		if (hrc != MF_PARSE_OK) die(mf_host_parse_strerror(hrc));
		if (held.users != prob.users || held.items != prob.items) die(mf_host_parse_strerror(MF_PARSE_THREE_INTS));
	}
	const double t1 = now();

	const size_t nl = (size_t) prob.users * (size_t) prob.features;
	const size_t nr = (size_t) prob.items * (size_t) prob.features;
	double *L = malloc(sizeof(double) * (nl ? nl : 1));
	double *R = malloc(sizeof(double) * (nr ? nr : 1));
	int32_t *best = malloc(sizeof(int32_t) * (size_t) (prob.users > 0 ? prob.users : 1));
	if (!L || !R || !best) die("Out of memory.");
	mf_host_init_factors(prob.users, prob.items, prob.features, L, R);
	const double t2 = now();

	int32_t *topn_items = NULL;
	if (topn) {
		topn_items = malloc(sizeof(int32_t) * (size_t) (prob.users > 0 ? prob.users : 1) * (size_t) topn);
		if (!topn_items) die("Out of memory.");
	}

	int device = 0;
	if (getenv("MATFACT_DEVICE")) device = atoi(getenv("MATFACT_DEVICE"));
	const char *mats = getenv("MATFACT_MATS");
	const char *devlist = getenv("MATFACT_DEVICES");   /* e.g. "0,1,2,3,4,5,6,7": row-shard over these GPUs */
	int rc, start_iter = 0;
	if (getenv("MATFACT_RESUME")) {
		if (mf_host_checkpoint_read(getenv("MATFACT_RESUME"), &prob, &start_iter, L, R) != 0)
			die("MATFACT_RESUME: cannot read the checkpoint or it belongs to another instance.");
	}
	if (biased && loss_every) {
		rc = run_biased_with_loss(&prob, have_held ? &held : NULL, L, R, best, device, loss_every, loss_tol, rank_cutoff, regularised,
		                          lambda_users, lambda_items);
	} else if (biased) {
		/* biases start at 0.0; L and R took the reference's random() stream for K = F above */
		double mu = 0.0;
		double *bu = calloc((size_t) (prob.users > 0 ? prob.users : 1), sizeof(double));
		double *bi = calloc((size_t) (prob.items > 0 ? prob.items : 1), sizeof(double));
		if (!bu || !bi) die("Out of memory.");
		rc = mf_backend_run_biased(&prob, L, R, bu, bi, &mu, best, lambda_users, lambda_items, device);
		free(bu);
		free(bi);
	} else if (loss_every) {
		rc = run_with_loss(&prob, have_held ? &held : NULL, L, R, best, device, loss_every, loss_tol, rank_cutoff, regularised,
		                   lambda_users, lambda_items, 0, 0.0);
	} else if (regularised) {
		rc = mf_backend_run_reg(&prob, L, R, best, lambda_users, lambda_items, device);
	} else if (topn) {
		rc = mf_backend_run_topn(&prob, L, R, topn, topn_items, NULL, device);
	} else if (similar) {
		rc = run_with_similar(&prob, L, R, best, device, similar, similar_metric, getenv("MATFACT_SIMILAR_OUT"));
	} else if (getenv("MATFACT_CHECKPOINT") || getenv("MATFACT_RESUME")) {
		rc = run_with_checkpoints(&prob, L, R, best, device, start_iter);
	} else if (mats) {
		rc = run_with_mats(mats, &prob, L, R, best, device);
	} else if (devlist) {
		int devs[16], nd = 0;
		for (const char *c = devlist; *c && nd < 16;) {
			char *stop;
			devs[nd++] = (int) strtol(c, &stop, 10);
			if (stop == c) die("MATFACT_DEVICES: expected a comma-separated list of device ordinals.");
			c = *stop == ',' ? stop + 1 : stop;
		}
		rc = mf_backend_run_multi(&prob, L, R, best, devs, nd);
	} else {
		rc = mf_backend_run_top1(&prob, L, R, best, device);   /* only the list is printed: no copy-back of L and R */
	}
	if (rc != MF_OK) {
		fprintf(stderr, "matFact (hip backend): %s %s\n", mf_backend_strerror(rc),
		        rc == MF_ERR_HIP ? mf_backend_last_hip_error() : "");
		die("GPU backend failed.");
	}
	const double t3 = now();

	if (topn)
		mf_host_write_topn(stdout, topn_items, prob.users, topn);
	else
		mf_host_write_out(stdout, best, prob.users);
	fflush(stdout);

	if (getenv("MATFACT_TIMING"))
		fprintf(stderr, "parse%s %.6f init %.6f gpu(run) %.6f total %.6f\n", cache_hit ? "(cache)" : "", t1 - t0, t2 - t1,
		        t3 - t2, now() - t0);
	free(best);
	free(topn_items);
	free(L);
	free(R);
	if (have_held) mf_host_free_problem(&held);
	mf_host_free_problem(&prob);
	return 0;
}
