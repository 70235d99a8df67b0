/*
 * matFact.c -- the drop-in command line: `matFact <file.in>` with the reference's argv handling, input
 * grammar, stdout format and error convention (matFact.c:61-137, util.c:7-10), the iteration loop and the
 * recommendation step running on an MI355X through the C ABI of include/matfact_hip.h.
 *
 * stdout carries ONLY the recommendations (one index per line), byte-identical to the reference's `.out`
 * files; timing goes to stderr and only when MATFACT_TIMING is set (the root-dir reference build appends a
 * `time : %f` line to stdout, benchmark.h:23; the hand-in build prints none).
 *
 * Top down: the options (one record, filled from the environment by one function; the combination rules are two tables),
 * the plan session (the one place a resident plan is opened and closed) with the stages that run over it, main().
 */
#define _POSIX_C_SOURCE 200809L
#include "../../include/matfact_hip.h"
#include "../../include/matfact_host.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

/* Every MATFACT_* variable the program reads: the mode options in the order they are examined, the path options, and the
 * accessories, which take part in no rule. */
enum { V_TOPN, V_LOSS, V_HELDOUT, V_RANK, V_SIMILAR, V_SIMILAR_OUT, V_LAMBDA, V_BIAS, V_MOMENTUM, V_WEIGHTS, V_BOUNDS, V_OPTIMIZER, V_SOLVER, V_IMPLICIT, V_ALS_CG, V_IMPLICIT_CG, V_ALS_BOX, V_DEVICES, V_MATS, V_CHECKPOINT, V_RESUME,
       V_DEVICE, V_MATS_ITERS, V_CHECKPOINT_EVERY, V_CACHE, V_TIMING, V_COUNT };
static const char *const cli_names[V_COUNT] = {
	"MATFACT_TOPN", "MATFACT_LOSS", "MATFACT_HELDOUT", "MATFACT_RANK", "MATFACT_SIMILAR", "MATFACT_SIMILAR_OUT", "MATFACT_LAMBDA",
	"MATFACT_BIAS", "MATFACT_MOMENTUM", "MATFACT_WEIGHTS", "MATFACT_BOUNDS", "MATFACT_OPTIMIZER", "MATFACT_SOLVER", "MATFACT_IMPLICIT", "MATFACT_ALS_CG", "MATFACT_IMPLICIT_CG", "MATFACT_ALS_BOX", "MATFACT_DEVICES", "MATFACT_MATS", "MATFACT_CHECKPOINT", "MATFACT_RESUME", "MATFACT_DEVICE",
	"MATFACT_MATS_ITERS", "MATFACT_CHECKPOINT_EVERY", "MATFACT_CACHE", "MATFACT_TIMING"};

struct cli_options {
	/* the variable's text, NULL when unset.  Used as they are: the paths MATFACT_HELDOUT=<file.in> (a second file with the
	 * same users and items), MATFACT_WEIGHTS=<file.in> (a second file with the same users, items and (row, col) pairs in the
	 * same order, whose values are the entries' confidence weights), _SIMILAR_OUT, _MATS, _CHECKPOINT, _RESUME, and _CACHE=<dir> (binary cache of parsed inputs keyed
	 * by the file's content; util.c:30-34 re-parses every run); MATFACT_TIMING only has to be set */
	const char *value[V_COUNT];
	int topn;             /* MATFACT_TOPN=N (1..MF_TOPN_MAX): N items per user on one line each instead of one (mf_host_write_topn) */
	int loss_every;       /* MATFACT_LOSS=every[,tol]: training (with MATFACT_HELDOUT also held-out) RMSE every `every` iterations */
	double loss_tol;      /* on stderr; with tol the run stops by the rule of mf_plan_iterate_monitored */
	int rank_cutoff;      /* MATFACT_RANK=N (>= 1): one more stderr line with hit rate, MRR and NDCG at N of the held-out entries */
	int similar;          /* MATFACT_SIMILAR=N[,dot|cosine] (1..MF_TOPN_MAX): the N nearest other items of every item, one line per */
	int similar_metric;   /* item, to MATFACT_SIMILAR_OUT; cosine unless said */
	int regularised;      /* MATFACT_LAMBDA=l[,li]: L2 regularisation, one number for both sides or users,items (finite, >= 0); */
	double lambda_users, lambda_items;   /* with MATFACT_LOSS one more stderr line: ||L||^2, ||R||^2, the objective at the end */
	int biased;           /* MATFACT_BIAS=1: a ~ mu + b_user + b_item + l.r on frozen columns; the file's K is the latent count F */
	int momentum;         /* MATFACT_MOMENTUM=b[,bi]: heavy-ball momentum, one number for both sides or users,items (finite, >= 0) */
	double beta_users, beta_items;
	int bounded;          /* MATFACT_BOUNDS=lo,hi[,lo_items,hi_items]: every finished row projected onto [lo, hi] (0,inf: non-negative */
	double lo_users, hi_users, lo_items, hi_items;   /* factors); one pair for both sides or users then items; the bias columns stay free */
	int adaptive;         /* MATFACT_OPTIMIZER=adam,eta[,beta1,beta2[,eps]] | rmsprop,eta[,rho[,eps]] | adagrad,eta[,eps]: a per-element */
	mf_adaptive optimizer;   /* adaptive step on both sides (eta, eps > 0; beta1, beta2, rho in [0, 1); defaults 0.9, 0.999, 1e-8) */
	int als;              /* MATFACT_SOLVER=als[,count]: the file's iters as ALS iterations (mf_plan_set_als: MF_ALS_RIDGE, or with */
	                      /* `count` MF_ALS_RIDGE_COUNT) from the reference's initialisation; lambda is MATFACT_LAMBDA's, default 0 */
	int implicit;         /* MATFACT_IMPLICIT=conf (finite, >= 0) next to MATFACT_SOLVER=als: the file's iters as implicit-feedback iterations */
	double conf;          /* (MF_ALS_IMPLICIT) at confidence 1 + conf * weight, and one objective line on stderr at the end */
	int als_cg;           /* MATFACT_ALS_CG=steps (1..MF_ALS_CG_MAX_STEPS) next to MATFACT_SOLVER: every row moves that many conjugate- */
	                      /* gradient steps per solve instead of being solved directly (mf_plan_set_als_cg); K up to 256 */
	int implicit_cg;      /* MATFACT_IMPLICIT_CG=steps (1..MF_ALS_CG_MAX_STEPS) next to MATFACT_IMPLICIT: the same for the implicit solve */
	                      /* (mf_plan_set_implicit_cg) */
	int als_box;          /* MATFACT_ALS_BOX=sweeps (1..MF_ALS_BOX_MAX_SWEEPS) next to MATFACT_SOLVER: every row is solved by that many */
	                      /* coordinate-descent sweeps inside MATFACT_BOUNDS' box instead of directly and clamped (mf_plan_set_als_box) */
	int device;           /* MATFACT_DEVICE=n: the GPU of a single-GPU run, default 0 */
	int devs[16], ndev;   /* MATFACT_DEVICES=0,1,...: row-shard over these GPUs of the process, at most 16 */
	const char *devices_error;   /* a non-number in it: said only where that path runs, after the input was read, as ever */
	int mats_iters;       /* MATFACT_MATS_ITERS=n: the dump also holds the state after each of the first n iterations, default 0 */
	int checkpoint_every; /* MATFACT_CHECKPOINT_EVERY=n: default 1000 */
};

/* a whole number from 1 to `max` at s, followed by the end of the text or by `sep`; *rest is where the number ended */
static int whole(const char *s, long max, char sep, const char **rest, int *out)
{
	char *stop;
	const long v = strtol(s, &stop, 10);
	*rest = stop;
	if (stop == s || v < 1 || v > max || (*stop && *stop != sep)) return 0;
	*out = (int) v;
	return 1;
}

static int number(const char *s, char sep, const char **rest, double *out)
{
	char *stop;
	*out = strtod(s, &stop);
	*rest = stop;
	return stop != s && (!*stop || *stop == sep);
}

/* The value format of mode option `v`: fills its fields of `o` and returns NULL, or returns the message. */
static const char *cli_value(int v, const char *s, struct cli_options *o)
{
	const char *rest, *bad;
	int ok;
	switch (v) {
	case V_TOPN:
		return whole(s, MF_TOPN_MAX, 0, &rest, &o->topn) ? NULL : "MATFACT_TOPN: expected a whole number from 1 to 32.";
	case V_LOSS:
		if (!whole(s, 2147483647L, ',', &rest, &o->loss_every)) return "MATFACT_LOSS: expected every[,tol] with every a whole number >= 1.";
		return !*rest || number(rest + 1, 0, &rest, &o->loss_tol) ? NULL : "MATFACT_LOSS: expected every[,tol] with tol a number.";
	case V_RANK:
		return whole(s, 2147483647L, 0, &rest, &o->rank_cutoff) ? NULL : "MATFACT_RANK: expected a whole number >= 1.";
	case V_SIMILAR:
		bad = "MATFACT_SIMILAR: expected N[,dot|cosine] with N a whole number from 1 to 32.";
		if (!whole(s, MF_TOPN_MAX, ',', &rest, &o->similar)) return bad;
		o->similar_metric = *rest && !strcmp(rest + 1, "dot") ? MF_SIMILAR_DOT : MF_SIMILAR_COSINE;
		return *rest && o->similar_metric == MF_SIMILAR_COSINE && strcmp(rest + 1, "cosine") ? bad : NULL;
	case V_LAMBDA:
		ok = number(s, ',', &rest, &o->lambda_users);
		o->lambda_items = o->lambda_users;
		if (ok && *rest) ok = number(rest + 1, 0, &rest, &o->lambda_items);
		o->regularised = ok && isfinite(o->lambda_users) && isfinite(o->lambda_items) && o->lambda_users >= 0.0 && o->lambda_items >= 0.0;
		return o->regularised ? NULL : "MATFACT_LAMBDA: expected l[,li] with l and li numbers >= 0.";
	case V_BIAS:
		o->biased = !strcmp(s, "1");
		return o->biased ? NULL : "MATFACT_BIAS: expected 1.";
	case V_MOMENTUM:
		ok = number(s, ',', &rest, &o->beta_users);
		o->beta_items = o->beta_users;
		if (ok && *rest) ok = number(rest + 1, 0, &rest, &o->beta_items);
		o->momentum = ok && isfinite(o->beta_users) && isfinite(o->beta_items) && o->beta_users >= 0.0 && o->beta_items >= 0.0;
		return o->momentum ? NULL : "MATFACT_MOMENTUM: expected b[,bi] with b and bi numbers >= 0.";
	case V_BOUNDS:
		ok = number(s, ',', &rest, &o->lo_users) && *rest && number(rest + 1, ',', &rest, &o->hi_users);
		o->lo_items = o->lo_users;
		o->hi_items = o->hi_users;
		if (ok && *rest) ok = number(rest + 1, ',', &rest, &o->lo_items) && *rest && number(rest + 1, 0, &rest, &o->hi_items);
		/* a NaN fails every comparison */
		o->bounded = ok && o->lo_users <= o->hi_users && o->lo_items <= o->hi_items;
		return o->bounded ? NULL : "MATFACT_BOUNDS: expected lo,hi[,lo_items,hi_items] with numbers lo <= hi.";
	case V_OPTIMIZER: {
		bad = "MATFACT_OPTIMIZER: expected adam,eta[,beta1,beta2[,eps]], rmsprop,eta[,rho[,eps]] or adagrad,eta[,eps] with eta, eps > 0 and beta1, beta2, rho in [0, 1).";
		mf_adaptive *a = &o->optimizer;
		const size_t n = strcspn(s, ",");
		a->kind = n == 4 && !strncmp(s, "adam", n) ? MF_OPT_ADAM : n == 7 && !strncmp(s, "rmsprop", n) ? MF_OPT_RMSPROP : n == 7 && !strncmp(s, "adagrad", n) ? MF_OPT_ADAGRAD : MF_OPT_NONE;
		a->beta1 = 0.9, a->beta2 = 0.999, a->eps = 1e-8;
		ok = a->kind != MF_OPT_NONE && s[n] && number(s + n + 1, ',', &rest, &a->eta);
		/* the betas the kind has: two, one or none, given together */
		if (ok && *rest && a->kind == MF_OPT_ADAM) ok = number(rest + 1, ',', &rest, &a->beta1) && *rest && number(rest + 1, ',', &rest, &a->beta2);
		else if (ok && *rest && a->kind == MF_OPT_RMSPROP) ok = number(rest + 1, ',', &rest, &a->beta2);
		if (ok && *rest) ok = number(rest + 1, 0, &rest, &a->eps);
		/* a NaN fails every comparison */
		o->adaptive = ok && isfinite(a->eta) && a->eta > 0.0 && isfinite(a->eps) && a->eps > 0.0 && a->beta1 >= 0.0 && a->beta1 < 1.0 &&
		              a->beta2 >= 0.0 && a->beta2 < 1.0;
		return o->adaptive ? NULL : bad;
	}
	case V_SOLVER:
		o->als = !strcmp(s, "als") ? MF_ALS_RIDGE : !strcmp(s, "als,count") ? MF_ALS_RIDGE_COUNT : MF_ALS_OFF;
		return o->als ? NULL : "MATFACT_SOLVER: expected als or als,count.";
	case V_IMPLICIT:
		o->implicit = number(s, 0, &rest, &o->conf) && isfinite(o->conf) && o->conf >= 0.0;
		if (!o->implicit) return "MATFACT_IMPLICIT: expected conf, a number >= 0.";
		if (o->als == MF_ALS_RIDGE_COUNT) return "MATFACT_IMPLICIT cannot be combined with MATFACT_SOLVER=als,count.";
		if (o->als == MF_ALS_RIDGE) o->als = MF_ALS_IMPLICIT;   /* unset: the needs row below says so */
		return NULL;
	case V_ALS_CG:
		return whole(s, MF_ALS_CG_MAX_STEPS, 0, &rest, &o->als_cg) ? NULL : "MATFACT_ALS_CG: expected a whole number from 1 to 256.";
	case V_IMPLICIT_CG:
		return whole(s, MF_ALS_CG_MAX_STEPS, 0, &rest, &o->implicit_cg) ? NULL : "MATFACT_IMPLICIT_CG: expected a whole number from 1 to 256.";
	case V_ALS_BOX:
		return whole(s, MF_ALS_BOX_MAX_SWEEPS, 0, &rest, &o->als_box) ? NULL : "MATFACT_ALS_BOX: expected a whole number from 1 to 256.";
	}
	return NULL;   /* MATFACT_HELDOUT, MATFACT_SIMILAR_OUT, MATFACT_WEIGHTS: any text */
}

/* The combination rules.  A mode option is examined only when it is set, in the order of the enum: its value format first,
 * then its rows of cli_needs, then its rows of cli_clashes, each in table order.  The first failure is the message. */
#define BIT(v) (1u << (v))
#define PATHS (BIT(V_DEVICES) | BIT(V_MATS) | BIT(V_CHECKPOINT) | BIT(V_RESUME))
#define COUNT(a) (sizeof(a) / sizeof((a)[0]))
struct cli_rule {
	int var;
	unsigned others;
	const char *message;
};
/* `var` needs every one of `others` (MATFACT_SIMILAR_OUT counts only when it is not empty) */
static const struct cli_rule cli_needs[] = {
	{V_HELDOUT, BIT(V_LOSS), "MATFACT_HELDOUT needs MATFACT_LOSS=every[,tol]."},
	{V_RANK, BIT(V_LOSS) | BIT(V_HELDOUT), "MATFACT_RANK needs MATFACT_HELDOUT=<file.in>."},
	{V_SIMILAR, BIT(V_SIMILAR_OUT), "MATFACT_SIMILAR needs MATFACT_SIMILAR_OUT=<path>."},
	{V_SIMILAR_OUT, BIT(V_SIMILAR), "MATFACT_SIMILAR_OUT needs MATFACT_SIMILAR=N[,dot|cosine]."},
	{V_IMPLICIT, BIT(V_SOLVER), "MATFACT_IMPLICIT needs MATFACT_SOLVER=als."},
	{V_ALS_CG, BIT(V_SOLVER), "MATFACT_ALS_CG needs MATFACT_SOLVER=als or als,count."},
	{V_IMPLICIT_CG, BIT(V_IMPLICIT), "MATFACT_IMPLICIT_CG needs MATFACT_IMPLICIT."},
	{V_ALS_BOX, BIT(V_SOLVER), "MATFACT_ALS_BOX needs MATFACT_SOLVER=als or als,count."},
};
/* `var` cannot be combined with any one of `others` (MATFACT_SIMILAR has two rows: it says two different things) */
static const struct cli_rule cli_clashes[] = {
	{V_TOPN, PATHS, "MATFACT_TOPN works on the single-GPU path only: unset MATFACT_DEVICES, MATFACT_MATS, MATFACT_CHECKPOINT and MATFACT_RESUME."},
	{V_LOSS, PATHS | BIT(V_TOPN), "MATFACT_LOSS works on the single-GPU path only: unset MATFACT_DEVICES, MATFACT_MATS, MATFACT_CHECKPOINT, MATFACT_RESUME and MATFACT_TOPN."},
	{V_SIMILAR, PATHS, "MATFACT_SIMILAR works on the single-GPU path only: unset MATFACT_DEVICES, MATFACT_MATS, MATFACT_CHECKPOINT and MATFACT_RESUME."},
	{V_SIMILAR, BIT(V_TOPN) | BIT(V_LOSS), "MATFACT_SIMILAR cannot be combined with MATFACT_TOPN or MATFACT_LOSS."},
	{V_LAMBDA, PATHS | BIT(V_TOPN) | BIT(V_SIMILAR), "MATFACT_LAMBDA works on the single-GPU path only: unset MATFACT_DEVICES, MATFACT_MATS, MATFACT_CHECKPOINT, MATFACT_RESUME, MATFACT_TOPN and MATFACT_SIMILAR."},
	{V_BIAS, PATHS | BIT(V_TOPN) | BIT(V_SIMILAR), "MATFACT_BIAS works on the single-GPU path only: unset MATFACT_DEVICES, MATFACT_MATS, MATFACT_CHECKPOINT, MATFACT_RESUME, MATFACT_TOPN and MATFACT_SIMILAR."},
	{V_MOMENTUM, PATHS | BIT(V_TOPN) | BIT(V_SIMILAR), "MATFACT_MOMENTUM works on the single-GPU path only: unset MATFACT_DEVICES, MATFACT_MATS, MATFACT_CHECKPOINT, MATFACT_RESUME, MATFACT_TOPN and MATFACT_SIMILAR."},
	{V_WEIGHTS, PATHS | BIT(V_TOPN) | BIT(V_SIMILAR), "MATFACT_WEIGHTS works on the single-GPU path only: unset MATFACT_DEVICES, MATFACT_MATS, MATFACT_CHECKPOINT, MATFACT_RESUME, MATFACT_TOPN and MATFACT_SIMILAR."},
	{V_BOUNDS, PATHS | BIT(V_TOPN) | BIT(V_SIMILAR), "MATFACT_BOUNDS works on the single-GPU path only: unset MATFACT_DEVICES, MATFACT_MATS, MATFACT_CHECKPOINT, MATFACT_RESUME, MATFACT_TOPN and MATFACT_SIMILAR."},
	{V_OPTIMIZER, PATHS | BIT(V_TOPN) | BIT(V_SIMILAR) | BIT(V_MOMENTUM), "MATFACT_OPTIMIZER works on the single-GPU path only and not with momentum: unset MATFACT_DEVICES, MATFACT_MATS, MATFACT_CHECKPOINT, MATFACT_RESUME, MATFACT_TOPN, MATFACT_SIMILAR and MATFACT_MOMENTUM."},
	{V_SOLVER, PATHS | BIT(V_SIMILAR) | BIT(V_MOMENTUM) | BIT(V_OPTIMIZER), "MATFACT_SOLVER works on the single-GPU path only and not with momentum or an optimizer: unset MATFACT_DEVICES, MATFACT_MATS, MATFACT_CHECKPOINT, MATFACT_RESUME, MATFACT_SIMILAR, MATFACT_MOMENTUM and MATFACT_OPTIMIZER."},
	{V_IMPLICIT, BIT(V_BIAS), "MATFACT_IMPLICIT cannot be combined with MATFACT_BIAS: the implicit solve has no frozen columns."},
	{V_ALS_CG, BIT(V_IMPLICIT), "MATFACT_ALS_CG cannot be combined with MATFACT_IMPLICIT: the implicit solve is the direct one."},
	{V_ALS_BOX, BIT(V_ALS_CG) | BIT(V_IMPLICIT_CG), "MATFACT_ALS_BOX cannot be combined with MATFACT_ALS_CG or MATFACT_IMPLICIT_CG: the box sweeps replace the direct solve."},
};

/* Fills `o` from the environment -- it opens no file and makes no GPU call -- and returns NULL, or the message to die with. */
static const char *cli_parse(struct cli_options *o)
{
	unsigned set = 0;
	memset(o, 0, sizeof(*o));
	for (int v = 0; v < V_COUNT; v++)
		if ((o->value[v] = getenv(cli_names[v])) != NULL) set |= BIT(v);
	const unsigned usable = o->value[V_SIMILAR_OUT] && !*o->value[V_SIMILAR_OUT] ? set & ~BIT(V_SIMILAR_OUT) : set;
	for (int v = V_TOPN; v <= V_ALS_BOX; v++) {
		const char *message = set & BIT(v) ? cli_value(v, o->value[v], o) : NULL;
		if (message) return message;
		if (!(set & BIT(v))) continue;
		for (size_t r = 0; r < COUNT(cli_needs); r++)
			if (cli_needs[r].var == v && (usable & cli_needs[r].others) != cli_needs[r].others) return cli_needs[r].message;
		for (size_t r = 0; r < COUNT(cli_clashes); r++)
			if (cli_clashes[r].var == v && (set & cli_clashes[r].others)) return cli_clashes[r].message;
	}
	/* the accessories parse leniently */
	o->device = o->value[V_DEVICE] ? atoi(o->value[V_DEVICE]) : 0;
	o->mats_iters = o->value[V_MATS_ITERS] ? atoi(o->value[V_MATS_ITERS]) : 0;
	o->checkpoint_every = o->value[V_CHECKPOINT_EVERY] ? atoi(o->value[V_CHECKPOINT_EVERY]) : 1000;
	if (o->checkpoint_every < 1) o->checkpoint_every = 1;
	for (const char *c = o->value[V_DEVICES]; c && *c && o->ndev < 16 && !o->devices_error;) {
		char *stop;
		o->devs[o->ndev++] = (int) strtol(c, &stop, 10);
		if (stop == c) o->devices_error = "MATFACT_DEVICES: expected a comma-separated list of device ordinals.";
		c = *stop == ',' ? stop + 1 : stop;
	}
	return NULL;
}

/* One resident single-GPU plan over a whole problem and the host buffers it reads: the only place that splits entries into
 * SoA form, fills an mf_shard and creates a plan.  session_close releases everything, whatever was acquired.
 * MATFACT_BIAS (here next to MATFACT_LOSS or MATFACT_MOMENTUM) is a preparation in front of the plan: the values are centred with the
 * training mean `mu` (one rounding each; the held-out ones later with the SAME mean), L and R -- the reference's
 * initialisation for K = F -- are packed to K = F + 2 by mf_backend_bias_pack with the biases at 0.0.  MATFACT_WEIGHTS makes
 * the plan a weighted one (mf_plan_create_weighted); `mu` stays the unweighted mean of the values. */
struct session {
	mf_plan *plan;
	int32_t *row, *col, *hrow, *hcol;   /* the training entries; the held-out ones, in buffers of their own */
	double *val, *hval, *wgt;           /* wgt: the entries' weights of MATFACT_WEIGHTS */
	double *Lp, *Rp, mu;                /* MATFACT_BIAS: the packed initial factors and the mean */
};

static int split_entries(const mf_problem *p, int32_t **row, int32_t **col, double **val)
{
	const size_t n = (size_t) (p->nnz ? p->nnz : 1);
	*row = malloc(sizeof(int32_t) * n);
	*col = malloc(sizeof(int32_t) * n);
	*val = malloc(sizeof(double) * n);
	if (!*row || !*col || !*val) return MF_ERR_NO_MEMORY;
	mf_host_split_entries(p->entries, p->nnz, *row, *col, *val);
	return MF_OK;
}

static int session_open(struct session *s, const struct cli_options *o, const mf_problem *p, const mf_problem *wts, const double *L,
                        const double *R)
{
	const int32_t F = p->features, K = o->biased ? F + 2 : F;
	memset(s, 0, sizeof(*s));
	int rc = split_entries(p, &s->row, &s->col, &s->val);
	if (rc == MF_OK && o->biased) {
		s->Lp = malloc(sizeof(double) * ((size_t) p->users * (size_t) K + 1));
		s->Rp = malloc(sizeof(double) * ((size_t) p->items * (size_t) K + 1));
		rc = s->Lp && s->Rp ? mf_backend_bias_mean(s->val, p->nnz, &s->mu) : MF_ERR_NO_MEMORY;
		for (int64_t i = 0; rc == MF_OK && i < p->nnz; i++) s->val[i] -= s->mu;
		if (rc == MF_OK) rc = mf_backend_bias_pack(L, NULL, p->users, F, 1, s->Lp);
		if (rc == MF_OK) rc = mf_backend_bias_pack(R, NULL, p->items, F, 0, s->Rp);
	}
	const mf_shard shard = {.users_total = p->users, .items = p->items, .features = K, .user_begin = 0, .user_count = p->users,
	                        .nnz = p->nnz, .row = s->row, .col = s->col, .val = s->val, .alpha = p->alpha, .device = o->device,
	                        .flags = MF_PLAN_DEFAULT};
	if (rc == MF_OK && wts) {
		s->wgt = malloc(sizeof(double) * (size_t) (p->nnz ? p->nnz : 1));
		for (int64_t i = 0; s->wgt && i < p->nnz; i++) s->wgt[i] = wts->entries[i].value;
		if (!s->wgt) rc = MF_ERR_NO_MEMORY;
	}
	if (rc == MF_OK) rc = mf_plan_create_weighted(&s->plan, &shard, s->wgt);   /* no weights: mf_plan_create in every respect */
	if (rc == MF_OK) rc = mf_plan_upload_factors(s->plan, o->biased ? s->Lp : L, o->biased ? s->Rp : R);
	return rc;
}

static void session_close(struct session *s)
{
	void *const owned[] = {s->row, s->col, s->val, s->hrow, s->hcol, s->hval, s->wgt, s->Lp, s->Rp};
	mf_plan_destroy(s->plan);
	for (size_t i = 0; i < COUNT(owned); i++) free(owned[i]);
}

/* MATFACT_CHECKPOINT / MATFACT_RESUME: steps that end on the multiples of checkpoint_every, (L, R, iterations done) written
 * after each but the last.  The final factors and recommendations are bit-identical to an uninterrupted run. */
static int loop_checkpointed(mf_plan *plan, const struct cli_options *o, const mf_problem *p, double *L, double *R, int done)
{
	const char *ck = o->value[V_CHECKPOINT];
	const int every = o->checkpoint_every;
	int rc = MF_OK;
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
	return rc;
}

/* MATFACT_MATS: the reference's debug dump format: the dense rating matrix, then L, R (printed K x I, i.e. un-transposed)
 * and B = L R^T with "%f " per element -- initially, after each of the first MATFACT_MATS_ITERS iterations (inst0.mats
 * holds 5) and at the end.  Every number printed comes from the GPU path. */
struct dump {
	FILE *f;
	double *B;   /* users x items */
};

static void mats_matrix(FILE *f, const char *title, const double *m, int rows, int cols, int transposed)
{
	fprintf(f, "%s\n", title);
	for (int i = 0; i < rows; i++) {
		for (int j = 0; j < cols; j++)
			fprintf(f, "%f ", transposed ? m[(size_t) j * rows + i] : m[(size_t) i * cols + j]);
		fprintf(f, "\n");
	}
}

static int mats_state(const struct dump *d, mf_plan *plan, const mf_problem *p, double *L, double *R, int initial)
{
	int rc = mf_plan_download_factors(plan, L, R);
	if (rc == MF_OK) rc = mf_plan_predict(plan, d->B);
	if (rc != MF_OK) return rc;
	mats_matrix(d->f, initial ? "Initial matrix L" : "Matrix L", L, p->users, p->features, 0);
	mats_matrix(d->f, initial ? "Initial matrix R" : "Matrix R", R, p->features, p->items, 1);
	mats_matrix(d->f, initial ? "Initial matrix B" : "Matrix B", d->B, p->users, p->items, 0);
	return MF_OK;
}

static int loop_dumped(mf_plan *plan, const struct cli_options *o, const mf_problem *p, double *L, double *R, const struct dump *d)
{
	const int shown = o->mats_iters > p->iters ? p->iters : o->mats_iters;
	int rc = mats_state(d, plan, p, L, R, 1);
	for (int it = 0; rc == MF_OK && it < shown; it++) {
		rc = mf_plan_iterate(plan, 1);
		if (rc == MF_OK) {
			fprintf(d->f, "Iter=%d\n", it);
			rc = mats_state(d, plan, p, L, R, 0);
		}
	}
	if (rc == MF_OK) rc = mf_plan_iterate(plan, p->iters - shown);
	if (rc == MF_OK) {
		fprintf(d->f, "Final:\n");
		rc = mats_state(d, plan, p, L, R, 0);
	}
	return rc;
}

/* MATFACT_LAMBDA with MATFACT_LOSS: the penalty's norms of the final factors and the objective at them */
static int report_penalty(mf_plan *plan, const struct cli_options *o)
{
	double lsq = 0.0, rsq = 0.0;
	mf_loss fin;
	int rc = mf_plan_penalty(plan, &lsq, &rsq, NULL, NULL);
	if (rc == MF_OK) rc = mf_plan_loss(plan, MF_LOSS_TRAIN, &fin, NULL);
	if (rc == MF_OK)
		fprintf(stderr, "penalty lambda %.17g %.17g users_sq %.17g items_sq %.17g objective %.17g\n", o->lambda_users, o->lambda_items,
		        lsq, rsq, (fin.sse + o->lambda_users * lsq) + o->lambda_items * rsq);
	return rc;
}

/* MATFACT_RANK: the metrics at `cutoff` of the held-out entries' ranks; `users` are their users in the caller's order */
static int report_ranks(mf_plan *plan, int cutoff, const int32_t *users, int64_t n)
{
	mf_rank_metrics m = {.hit_rate = NAN, .mrr = NAN, .ndcg = NAN};   /* an empty held-out file: nothing is evaluated */
	int rc = MF_OK;
	if (n > 0) {
		int32_t *ranks = malloc(sizeof(int32_t) * (size_t) n);
		rc = ranks ? mf_plan_rank_heldout(plan, ranks) : MF_ERR_NO_MEMORY;
		if (rc == MF_OK) rc = mf_backend_rank_metrics(ranks, users, n, cutoff, &m);
		free(ranks);
	}
	if (rc == MF_OK)
		fprintf(stderr, "heldout_rank cutoff %d evaluated %lld masked %lld nan %lld users %lld hits %lld hit_rate %.17g mrr %.17g ndcg %.17g\n",
		        cutoff, (long long) m.evaluated, (long long) m.masked, (long long) m.nan, (long long) m.users, (long long) m.hits,
		        m.hit_rate, m.mrr, m.ndcg);
	return rc;
}

/* MATFACT_SIMILAR: the neighbours of every item by the trained R, to MATFACT_SIMILAR_OUT */
static int write_similar(mf_plan *plan, const struct cli_options *o, int32_t items)
{
	int32_t *near = malloc(sizeof(int32_t) * (size_t) (items > 0 ? items : 1) * (size_t) o->similar);
	int rc = near ? mf_plan_similar_items(plan, o->similar_metric, NULL, items, o->similar, near, NULL) : MF_ERR_NO_MEMORY;
	if (rc == MF_OK) {
		FILE *f = fopen(o->value[V_SIMILAR_OUT], "w");
		if (!f || mf_host_write_topn(f, near, items, o->similar) != 0) rc = MF_ERR_ARGUMENT;
		if (f && fclose(f) == EOF) rc = MF_ERR_ARGUMENT;
	}
	free(near);
	return rc;
}

/* MATFACT_IMPLICIT: the all-pairs objective of the final factors, ((all_sq + observed) + lambda_users ||L||^2) + lambda_items ||R||^2 */
static int report_implicit(mf_plan *plan, const struct cli_options *o)
{
	mf_implicit_objective ob;
	double us = 0.0, is = 0.0;
	int rc = mf_plan_implicit_objective(plan, &ob);
	if (rc == MF_OK) rc = mf_plan_penalty(plan, &us, &is, NULL, NULL);
	if (rc == MF_OK)
		fprintf(stderr, "implicit conf %.17g all_sq %.17g observed %.17g users_sq %.17g items_sq %.17g objective %.17g\n", o->conf, ob.all_sq,
		        ob.observed, us, is, ((ob.all_sq + ob.observed) + o->lambda_users * us) + o->lambda_items * is);
	return rc;
}

/* Every mode that needs a resident plan, as stages over one session: configure, exactly one loop, the reports on stderr,
 * the outputs.  `d` is the open dump of MATFACT_MATS or NULL; `done` counts the iterations a checkpoint already holds. */
static int run_session(const struct cli_options *o, const mf_problem *p, const mf_problem *held, const mf_problem *wts, double *L, double *R,
                       int32_t *best, int32_t *topn_items, int done, const struct dump *d)
{
	struct session s;
	const int cap = o->loss_every ? p->iters / o->loss_every + 2 : 0;
	mf_loss_point *trace = cap ? malloc(sizeof(mf_loss_point) * (size_t) cap) : NULL;
	const int checkpointed = o->value[V_CHECKPOINT] || o->value[V_RESUME];
	int points = 0;
	int rc = session_open(&s, o, p, wts, L, R);
	if (rc == MF_OK && cap && !trace) rc = MF_ERR_NO_MEMORY;
	/* configure: the held-out set, regularisation, the frozen columns of the biases, momentum, the box, the adaptive step */
	if (rc == MF_OK && held) rc = split_entries(held, &s.hrow, &s.hcol, &s.hval);
	for (int64_t i = 0; rc == MF_OK && held && o->biased && i < held->nnz; i++) s.hval[i] -= s.mu;
	if (rc == MF_OK && held) rc = mf_plan_set_heldout(s.plan, held->nnz, s.hrow, s.hcol, s.hval);
	if (rc == MF_OK && o->regularised) rc = mf_plan_set_regularization(s.plan, o->lambda_users, o->lambda_items);
	if (rc == MF_OK && o->biased) rc = mf_plan_set_frozen_columns(s.plan, p->features + 1, p->features);
	if (rc == MF_OK && o->momentum) rc = mf_plan_set_momentum(s.plan, o->beta_users, o->beta_items);
	/* the box covers the file's K columns: all of them, or with MATFACT_BIAS the latent F in front of the two bias columns */
	if (rc == MF_OK && o->bounded) rc = mf_plan_set_bounds(s.plan, 1, o->lo_users, o->hi_users, p->features);
	if (rc == MF_OK && o->bounded) rc = mf_plan_set_bounds(s.plan, 0, o->lo_items, o->hi_items, p->features);
	/* the adaptive step, the same rule on both sides */
	if (rc == MF_OK && o->adaptive) rc = mf_plan_set_adaptive(s.plan, 1, &o->optimizer);
	if (rc == MF_OK && o->adaptive) rc = mf_plan_set_adaptive(s.plan, 0, &o->optimizer);
	/* the solver: ALS in place of the gradient step */
	if (rc == MF_OK && o->implicit) rc = mf_plan_set_confidence(s.plan, o->conf);
	if (rc == MF_OK && o->als_cg) rc = mf_plan_set_als_cg(s.plan, o->als_cg);   /* first: K may lie in 129 .. 256 */
	if (rc == MF_OK && o->implicit_cg) rc = mf_plan_set_implicit_cg(s.plan, o->implicit_cg);
	if (rc == MF_OK && o->als_box) rc = mf_plan_set_als_box(s.plan, o->als_box);
	if (rc == MF_OK && o->als) rc = mf_plan_set_als(s.plan, o->als);
	/* loop */
	if (rc == MF_OK) {
		if (o->loss_every) rc = mf_plan_iterate_monitored(s.plan, p->iters, o->loss_every, o->loss_tol, trace, cap, &points, &done);
		else if (checkpointed) rc = loop_checkpointed(s.plan, o, p, L, R, done);
		else if (d) rc = loop_dumped(s.plan, o, p, L, R, d);
		else rc = mf_plan_iterate(s.plan, p->iters);
	}
	/* report, next to MATFACT_LOSS only (MATFACT_RANK needs it by the rules; MATFACT_BIAS with MATFACT_MOMENTUM runs here
	 * without it and reports nothing) */
	for (int i = 0; rc == MF_OK && i < points && i < cap; i++) {
		fprintf(stderr, "iter %d train_rmse %.17g", trace[i].iter,
		        trace[i].train.count > 0 ? sqrt(trace[i].train.sse / (double) trace[i].train.count) : NAN);
		if (held && held->nnz > 0) fprintf(stderr, " heldout_rmse %.17g", sqrt(trace[i].heldout.sse / (double) trace[i].heldout.count));
		fprintf(stderr, "\n");
	}
	if (rc == MF_OK && o->biased && o->loss_every) fprintf(stderr, "bias mu %.17g\n", s.mu);
	if (rc == MF_OK && o->regularised && o->loss_every) rc = report_penalty(s.plan, o);
	if (rc == MF_OK && o->rank_cutoff) rc = report_ranks(s.plan, o->rank_cutoff, s.hrow, held->nnz);
	if (rc == MF_OK && o->implicit) rc = report_implicit(s.plan, o);
	/* outputs */
	if (rc == MF_OK) rc = o->topn ? mf_plan_recommend_topn(s.plan, o->topn, topn_items, NULL) : mf_plan_recommend(s.plan, best);   /* MATFACT_TOPN comes here with MATFACT_SOLVER only */
	if (rc == MF_OK && o->similar) rc = write_similar(s.plan, o, p->items);
	if (rc == MF_OK && checkpointed) rc = mf_plan_download_factors(s.plan, L, R);
	session_close(&s);
	free(trace);
	return rc;
}

/* MATFACT_MATS around the session: the dump file, its dense B and the rating matrix A, written before the plan exists */
static int run_with_mats(const struct cli_options *o, const mf_problem *p, double *L, double *R, int32_t *best)
{
	/* the dense A and B of the dump exist only for small instances (mf_plan_predict refuses more than 2^26 elements);
	 * indices are checked BEFORE A is filled: the parser does not range-check them, only the device build does */
	const size_t nb = (size_t) p->users * (size_t) p->items;
	if (p->users < 0 || p->items < 0 || nb > ((size_t) 1 << 26)) return MF_ERR_UNSUPPORTED;
	for (int64_t n = 0; n < p->nnz; n++)
		if (p->entries[n].row < 0 || p->entries[n].row >= p->users || p->entries[n].col < 0 || p->entries[n].col >= p->items)
			return MF_ERR_ARGUMENT;
	struct dump d = {fopen(o->value[V_MATS], "w"), calloc(nb ? nb : 1, sizeof(double))};
	int rc = !d.f ? MF_ERR_ARGUMENT : !d.B ? MF_ERR_NO_MEMORY : MF_OK;
	if (rc == MF_OK) {
		for (int64_t n = 0; n < p->nnz; n++) d.B[(size_t) p->entries[n].row * p->items + p->entries[n].col] = p->entries[n].value;
		mats_matrix(d.f, "Initial matrix A", d.B, p->users, p->items, 0);
		rc = run_session(o, p, NULL, NULL, L, R, best, NULL, 0, &d);
	}
	free(d.B);
	if (d.f && fclose(d.f) == EOF && rc == MF_OK) rc = MF_ERR_ARGUMENT;
	return rc;
}

/* util.c:7-10 */
static void die(const char *error)
{
	fprintf(stderr, "Error: %s\n", error);
	exit(-1);
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
	/* every option is checked before the input is read: a refused run prints nothing on stdout */
	struct cli_options o;
	const char *refusal = cli_parse(&o);
	if (refusal) die(refusal);
	const double t0 = now();

	mf_problem prob, held, wts;
	int cache_hit = 0;
	const int prc = mf_host_parse_file_cached(argv[1], o.value[V_CACHE], &prob, &cache_hit);
	if (prc != MF_PARSE_OK) die(mf_host_parse_strerror(prc));
	const int have_held = o.value[V_HELDOUT] != NULL;
	if (have_held) {
		const int hrc = mf_host_parse_file(o.value[V_HELDOUT], &held);
		if (hrc != MF_PARSE_OK) die(mf_host_parse_strerror(hrc));
		if (held.users != prob.users || held.items != prob.items) die(mf_host_parse_strerror(MF_PARSE_THREE_INTS));
	}
	/* MATFACT_WEIGHTS: the same grammar; its values are the weights of the input's entries, pair by pair */
	const int have_wts = o.value[V_WEIGHTS] != NULL;
	if (have_wts) {
		const int wrc = mf_host_parse_file(o.value[V_WEIGHTS], &wts);
		if (wrc != MF_PARSE_OK) die(mf_host_parse_strerror(wrc));
		int same = wts.users == prob.users && wts.items == prob.items && wts.nnz == prob.nnz;
		for (int64_t n = 0; same && n < prob.nnz; n++)
			same = wts.entries[n].row == prob.entries[n].row && wts.entries[n].col == prob.entries[n].col;
		if (!same) die("MATFACT_WEIGHTS: the file must hold the input's users, items and (row, col) pairs, in the input's order.");
	}
	const double t1 = now();

	const size_t nl = (size_t) prob.users * (size_t) prob.features;
	const size_t nr = (size_t) prob.items * (size_t) prob.features;
	const size_t nu = (size_t) (prob.users > 0 ? prob.users : 1), ni = (size_t) (prob.items > 0 ? prob.items : 1);
	double *L = malloc(sizeof(double) * (nl ? nl : 1));
	double *R = malloc(sizeof(double) * (nr ? nr : 1));
	int32_t *best = malloc(sizeof(int32_t) * nu);
	if (!L || !R || !best) die("Out of memory.");
	mf_host_init_factors(prob.users, prob.items, prob.features, L, R);
	const double t2 = now();

	int32_t *topn_items = o.topn ? malloc(sizeof(int32_t) * nu * (size_t) o.topn) : NULL;
	if (o.topn && !topn_items) die("Out of memory.");
	int rc, start_iter = 0;
	if (o.value[V_RESUME] && mf_host_checkpoint_read(o.value[V_RESUME], &prob, &start_iter, L, R) != 0)
		die("MATFACT_RESUME: cannot read the checkpoint or it belongs to another instance.");
	/*
	 * The rules of cli_parse leave mode options or path options, never both.  Among the path options the priority is silent:
	 * MATFACT_CHECKPOINT / MATFACT_RESUME win over MATFACT_MATS, which wins over MATFACT_DEVICES (and MATFACT_RESUME is read
	 * above whenever it is set).  MATFACT_LOSS, MATFACT_SIMILAR, MATFACT_WEIGHTS, MATFACT_BOUNDS, MATFACT_OPTIMIZER, MATFACT_SOLVER, MATFACT_BIAS with MATFACT_MOMENTUM, the checkpoints and the dump need a resident plan and run as
	 * a session, which splits the entries once; the rest goes through the level-1 calls, which take the entries as they are.
	 */
	if (o.loss_every || o.similar || have_wts || o.bounded || o.adaptive || o.als || o.value[V_CHECKPOINT] || o.value[V_RESUME] || (o.momentum && o.biased)) {
		rc = run_session(&o, &prob, have_held ? &held : NULL, have_wts ? &wts : NULL, L, R, best, topn_items, start_iter, NULL);
	} else if (o.biased) {
		/* biases start at 0.0; L and R took the reference's random() stream for K = F above */
		double mu = 0.0;
		double *bu = calloc(nu, sizeof(double)), *bi = calloc(ni, sizeof(double));
		if (!bu || !bi) die("Out of memory.");
		rc = mf_backend_run_biased(&prob, L, R, bu, bi, &mu, best, o.lambda_users, o.lambda_items, o.device);
		free(bu);
		free(bi);
	} else if (o.momentum) {
		rc = mf_backend_run_momentum(&prob, L, R, best, o.lambda_users, o.lambda_items, o.beta_users, o.beta_items, o.device);
	} else if (o.regularised) {
		rc = mf_backend_run_reg(&prob, L, R, best, o.lambda_users, o.lambda_items, o.device);
	} else if (o.topn) {
		rc = mf_backend_run_topn(&prob, L, R, o.topn, topn_items, NULL, o.device);
	} else if (o.value[V_MATS]) {
		rc = run_with_mats(&o, &prob, L, R, best);
	} else if (o.value[V_DEVICES]) {
		if (o.devices_error) die(o.devices_error);
		rc = mf_backend_run_multi(&prob, L, R, best, o.devs, o.ndev);
	} else {
		rc = mf_backend_run_top1(&prob, L, R, best, o.device);   /* only the list is printed: no copy-back of L and R */
	}
	if (rc != MF_OK) {
		fprintf(stderr, "matFact (hip backend): %s %s\n", mf_backend_strerror(rc), rc == MF_ERR_HIP ? mf_backend_last_hip_error() : "");
		die("GPU backend failed.");
	}
	const double t3 = now();

	if (o.topn)
		mf_host_write_topn(stdout, topn_items, prob.users, o.topn);
	else
		mf_host_write_out(stdout, best, prob.users);
	fflush(stdout);

	if (o.value[V_TIMING])
		fprintf(stderr, "parse%s %.6f init %.6f gpu(run) %.6f total %.6f\n", cache_hit ? "(cache)" : "", t1 - t0, t2 - t1, t3 - t2,
		        now() - t0);
	free(best);
	free(topn_items);
	free(L);
	free(R);
	if (have_held) mf_host_free_problem(&held);
	if (have_wts) mf_host_free_problem(&wts);
	mf_host_free_problem(&prob);
	return 0;
}
