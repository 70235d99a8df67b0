// als_box_rule_main -- the solver rule (csrc/mf_schedule.h: als_solver) with the box sweeps of mf_plan_set_als_box, one line per
// kind x als_cg in {0, 3} x implicit_cg in {0, 3} x als_box in {0, 3} (tests/test_als_box.py):
//   solver kind als_cg implicit_cg als_box : conjugate gradient?, implicit?, steps, widest K, box sweeps
// and per kind x als_cg x implicit_cg what the three-argument call returns, the call of before the sweeps:
//   three kind als_cg implicit_cg : conjugate gradient?, implicit?, steps, widest K, box sweeps
#include <cstdio>

#include "../recommender-system_amd/csrc/mf_schedule.h"

int main()
{
	for (int kind : {0, 1, 2, 4})   // MF_ALS_OFF, RIDGE, RIDGE_COUNT, IMPLICIT
		for (int als_cg : {0, 3})
			for (int implicit_cg : {0, 3}) {
				for (int als_box : {0, 3}) {
					const mf_sched::AlsSolver s = mf_sched::als_solver(kind, als_cg, implicit_cg, als_box);
					printf("solver %d %d %d %d %d %d %d %d %d\n", kind, als_cg, implicit_cg, als_box, (int) s.cg, (int) s.implicit, s.steps, s.max_k,
					       s.box_sweeps);
				}
				const mf_sched::AlsSolver t = mf_sched::als_solver(kind, als_cg, implicit_cg);
				printf("three %d %d %d %d %d %d %d %d\n", kind, als_cg, implicit_cg, (int) t.cg, (int) t.implicit, t.steps, t.max_k, t.box_sweeps);
			}
	return 0;
}
