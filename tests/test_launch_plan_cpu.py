"""rcu_amd.steps.launch_plan: the one scheduling policy of the one-process predict steps and the sharded runners, as plain values.  The
literal launch lists below were recorded from the step and runner loops that the plan replaced (a recording stand-in for StreamLanes), so
they pin the lanes, groups, weight-scaling position and TTA folds that the bytes of the outputs depend on."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rcu_amd import distributed as rdist  # noqa: E402
from rcu_amd.steps import launch_plan  # noqa: E402


def test_mc_passes_run_in_balanced_groups_over_the_lanes_after_the_weight_scaling_pass():
    jobs = list(range(21))
    assert launch_plan(jobs, (0,), 20, group=4, lanes=2) == [
        ('ws', 0, 0, (0,)), ('passes', 0, 0, (1, 2, 3, 4)), ('passes', 1, 0, (5, 6, 7, 8)), ('passes', 0, 0, (9, 10, 11, 12)),
        ('passes', 1, 0, (13, 14, 15, 16)), ('passes', 0, 0, (17, 18)), ('passes', 1, 0, (19, 20))]
    jobs = list(range(6))
    assert launch_plan(jobs, (0,), 5, group=4, lanes=1) == [('ws', 0, 0, (0,)), ('passes', 0, 0, (1, 2, 3, 4)), ('passes', 0, 0, (5,))]
    assert launch_plan(jobs, (0,), 5, group=4, lanes=2) == [('ws', 0, 0, (0,)), ('passes', 0, 0, (1, 2, 3)), ('passes', 1, 0, (4, 5))]
    assert launch_plan(jobs, (0,), 5, group=2, lanes=2) == [
        ('ws', 0, 0, (0,)), ('passes', 0, 0, (1, 2)), ('passes', 1, 0, (3, 4)), ('passes', 0, 0, (5,))]
    assert launch_plan([0, 1], (0,), 1, group=4, lanes=1) == [('ws', 0, 0, (0,)), ('passes', 0, 0, (1,))]
    assert launch_plan(list(range(1, 6)), (0,), 5, group=4, lanes=2) == [('passes', 0, 0, (1, 2, 3)), ('passes', 1, 0, (4, 5))]
    assert launch_plan([0], (0,), 1, group=4, lanes=2) == [('ws', 0, 0, (0,))]


def test_a_rank_of_a_world_of_eight_starts_on_the_lane_of_its_step():
    runner = rdist.ShardedMcRunner(None, 20, ws_pass=True, rank=0, world=8, engine=object())
    assert runner.jobs_of(1, 0) == [3, 11, 19] and runner.jobs_of(5, 2) == [1, 9, 17]
    assert launch_plan([3, 11, 19], (0,), 20, group=4, lanes=2, first=1) == [('passes', 1, 0, (3, 11)), ('passes', 0, 0, (19,))]
    assert launch_plan([1, 9, 17], (0,), 20, group=4, lanes=2, first=5) == [('passes', 1, 0, (1, 9)), ('passes', 0, 0, (17,))]


def test_ensemble_members_keep_their_lane():
    assert launch_plan(range(1, 11), lanes=2, members=True) == [('member', (j - 1) % 2, 0, (j,)) for j in range(1, 11)]
    # a rank of a world of eight: members 2 and 10 stay on lane 1 whatever step the rotation hands them over in
    assert launch_plan([2, 10], lanes=2, first=1, members=True) == [('member', 1, 0, (2,)), ('member', 1, 0, (10,))]


def test_tta_elements_rotate_their_first_lane_and_fold_on_every_lane_they_used():
    assert launch_plan(list(range(13)), (0, 1, 2, 3), 3, group=2, lanes=2) == [
        ('ws', 0, 0, (0,)), ('passes', 0, 0, (1, 2)), ('passes', 1, 0, (3,)),
        ('passes', 1, 1, (4, 5)), ('passes', 0, 1, (6,)), ('fold', 0, 1, ()), ('fold', 1, 1, ()),
        ('passes', 0, 2, (7, 8)), ('passes', 1, 2, (9,)), ('fold', 0, 2, ()), ('fold', 1, 2, ()),
        ('passes', 1, 3, (10, 11)), ('passes', 0, 3, (12,)), ('fold', 0, 3, ()), ('fold', 1, 3, ())]
    # T = 0: one eval-mode pass per transform
    assert launch_plan(list(range(5)), (0, 1, 2, 3), 1, group=2, lanes=2) == [
        ('ws', 0, 0, (0,)), ('passes', 0, 0, (1,)), ('passes', 1, 1, (2,)), ('fold', 1, 1, ()), ('passes', 0, 2, (3,)), ('fold', 0, 2, ()),
        ('passes', 1, 3, (4,)), ('fold', 1, 3, ())]


def test_every_job_is_launched_once():
    for world in (1, 2, 8):
        for step in range(4):
            runner = rdist.ShardedTtaMcRunner(None, ['identity', 'flip_h', 'rot180'], 5, rank=0, world=world, seed=1)
            launched = []
            for rank in range(world):
                plan = launch_plan(runner.jobs_of(step, rank), runner.elements, runner.per_element, 2, 2, first=step if world > 1 else 0)
                assert all(lane in (0, 1) for _, lane, _, _ in plan)
                launched += [j for kind, _, _, jobs in plan if kind != 'fold' for j in jobs]
            assert sorted(launched) == runner.job_list()
