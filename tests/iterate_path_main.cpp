// iterate_path_main -- how an iteration runs by csrc/mf_schedule.h (iterate_path, toy_lds_bytes, toy_kmax), on the cases
// read from stdin, one line out per line in (tests/test_iterate_path.py).  The mode is the first argument:
//   path:  rows toy_bytes <rest>   the inputs of the rule as they are
//   plan:  users items <rest>      a plan's shape: rows = users + items, toy_bytes = the unweighted toy_lds_bytes
//          <rest> = nnz K iters als whole timing adaptive es extreme resident graph graph_max
//          out: the inputs as the rule saw them (rows toy_bytes nnz K iters, the eight flags, graph_max) : loop replays eager
//   shape: users items K nnz weighted threads   out: toy_lds_bytes toy_kmax
// the loop as the value of the enum.
#include <cstdio>
#include <cstring>

#include "../recommender-system_amd/csrc/mf_schedule.h"

int main(int argc, char **argv)
{
	const char *mode = argc > 1 ? argv[1] : "";
	if (!strcmp(mode, "shape")) {
		int users, items, K, weighted, threads;
		long long nnz;
		while (scanf("%d %d %d %lld %d %d", &users, &items, &K, &nnz, &weighted, &threads) == 6)
			printf("%zu %d\n", mf_sched::toy_lds_bytes(users, items, K, nnz, weighted != 0), mf_sched::toy_kmax(K, threads));
		return 0;
	}
	const bool plan = !strcmp(mode, "plan");
	if (!plan && strcmp(mode, "path")) return 2;
	long long a, b;
	while (scanf("%lld %lld", &a, &b) == 2) {
		mf_sched::IterateInput in;
		int als, whole, timing, adaptive, es, extreme, resident, graph;
		if (scanf("%lld %d %d %d %d %d %d %d %d %d %d %lf", &in.nnz, &in.K, &in.iters, &als, &whole, &timing, &adaptive, &es, &extreme,
		          &resident, &graph, &in.graph_max) != 12)
			return 3;
		in.rows = plan ? a + b : a;
		in.toy_bytes = plan ? mf_sched::toy_lds_bytes((int) a, (int) b, in.K, in.nnz) : (size_t) b;
		in.als = als, in.whole = whole, in.timing = timing, in.adaptive = adaptive;
		in.es_mode = es, in.extreme = extreme, in.resident = resident, in.graph = graph;
		const mf_sched::IteratePath p = mf_sched::iterate_path(in);
		printf("%lld %zu %lld %d %d %d %d %d %d %d %d %d %d %.17g : %d %d %d\n", in.rows, in.toy_bytes, in.nnz, in.K, in.iters, (int) in.als,
		       (int) in.whole, (int) in.timing, (int) in.adaptive, (int) in.es_mode, (int) in.extreme, (int) in.resident, (int) in.graph,
		       in.graph_max, (int) p.loop, p.replays, p.eager);
	}
	return 0;
}
