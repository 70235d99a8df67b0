// launch_choice_main -- the launch-time choice of csrc/mf_schedule.h (form, flavour, geometry of a sweep's main launch) on
// every combination of its inputs, one line each (tests/test_launch_choice.py):
//   coop_all use_db use_pair has_pipelined K n_short nrows decay momentum weighted few_rows : form flavour geometry
// the three results as the values of the enums.
#include <cstdio>

#include "../recommender-system_amd/csrc/mf_schedule.h"

int main()
{
	const int rows[2] = {262144, 262145};
	for (int bits = 0; bits < 256; ++bits) {
		const bool coop_all = bits & 1, use_db = bits & 2, use_pair = bits & 4, has_pf = bits & 8;
		const bool decay = bits & 16, momentum = bits & 32, weighted = bits & 64, few_rows = bits & 128;
		for (int K : {128, 256})
			for (int n_short : rows)
				for (int nrows : rows) {
					const bool pf = mf_sched::single_wave_pipelined(has_pf, K, n_short, nrows);
					const mf_sched::Form form = mf_sched::launch_form(coop_all, use_db, use_pair, pf);
					printf("%d %d %d %d %d %d %d %d %d %d %d : %d %d %d\n", (int) coop_all, (int) use_db, (int) use_pair, (int) has_pf, K,
					       n_short, nrows, (int) decay, (int) momentum, (int) weighted, (int) few_rows, (int) form,
					       (int) mf_sched::launch_flavour(weighted, momentum, decay), (int) mf_sched::launch_geometry(form, few_rows));
				}
	}
	return 0;
}
