"""The plan of a covariance-column pass (slam_toolbox_amd/csrc/covariance_columns_plan.hpp) on hand-written assembly trees, through
the stand-alone program tests/covariance_columns_plan_check.cpp: per query column exactly one front per level from the query's
front to the root and none elsewhere -- the reason every (row, column) of the right-hand sides has one writer per launch.  No GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cols") / "covariance_columns_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(HERE, "covariance_columns_plan_check.cpp"), "-o", exe],
                   check=True)

    def run(tree, queries):
        parent, level, sn_of_elim, elim_of_free = tree
        words = [len(parent), *parent, *level, len(sn_of_elim), *sn_of_elim, *elim_of_free, len(queries), *queries]
        r = subprocess.run([exe], input=" ".join(str(w) for w in words) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        f = r.stdout.split()
        if f[0] == "fail":
            return None
        assert f[0] == "ok"
        n_path, n_levels, at = int(f[1]), int(f[2]), 3
        levels = []
        for _ in range(n_levels):
            count = int(f[at])
            at += 1
            levels.append([(int(f[at + 2 * t]), int(f[at + 2 * t + 1], 16)) for t in range(count)])
            at += 2 * count
        query_front = [int(v) for v in f[at:at + len(queries)]]
        at += len(queries)
        front_mask = [int(v, 16) for v in f[at:]]
        assert len(front_mask) == len(parent)
        return dict(n_path=n_path, levels=levels, query_front=query_front, front_mask=front_mask)
    return run


def check_one_front_per_level(tree, queries, out):
    """the property itself, from the tree alone: returns the fronts of every query's path"""
    parent, level, sn_of_elim, elim_of_free = tree
    n_levels = max(level) + 1
    paths = []
    for k, q in enumerate(queries):
        path = []
        front = sn_of_elim[elim_of_free[q]] if q >= 0 else -1
        assert out["query_front"][k] == front
        while front >= 0:
            path.append(front)
            front = parent[front]
        paths.append(path)
        carried = [[f for f, mask in out["levels"][l] if (mask >> k) & 1] for l in range(n_levels)]
        on_path_levels = {level[f] for f in path}
        assert len(on_path_levels) == len(path), "two fronts of a path on one level"
        for l in range(n_levels):
            assert len(carried[l]) <= 1, (k, l, carried[l])                  # one writer per (row, column) and launch
            assert carried[l] == [f for f in path if level[f] == l], (k, l)
    listed = [f for lv in out["levels"] for f, _ in lv]
    union = sorted({f for p in paths for f in p})
    assert sorted(listed) == union and len(listed) == len(set(listed)) and out["n_path"] == len(union)
    for l, lv in enumerate(out["levels"]):
        assert all(level[f] == l for f, _ in lv)
        assert [f for f, _ in lv] == sorted(f for f, _ in lv)
        assert all(mask == out["front_mask"][f] and mask != 0 for f, mask in lv)
    assert all(out["front_mask"][f] == 0 for f in range(len(parent)) if f not in union)
    return paths


# level 0: fronts 0 1 2 3 and 4 (a leaf right under the root: its path skips level 1); level 1: 5 (children 0, 1), 6 (children 2, 3);
# level 2: the root 7.  Front k eliminates positions 2 k and 2 k + 1; free node f sits at elimination position 15 - f.
TREE = ([5, 5, 6, 6, 7, 7, 7, -1], [0, 0, 0, 0, 0, 1, 1, 2], [k // 2 for k in range(16)], [15 - f for f in range(16)])


def free_of_front(front, which=0):
    return 15 - (2 * front + which)


def test_single_front_tree(plan):
    tree = ([-1], [0], [0, 0, 0, 0], [2, 0, 3, 1])
    out = plan(tree, [1, 3])
    assert out["levels"] == [[(0, 0b11)]] and out["n_path"] == 1
    check_one_front_per_level(tree, [1, 3], out)


def test_query_in_the_root(plan):
    q = [free_of_front(7)]
    out = plan(TREE, q)
    assert out["levels"] == [[], [], [(7, 1)]] and out["query_front"] == [7]
    check_one_front_per_level(TREE, q, out)


def test_leaf_to_root_and_a_path_that_skips_a_level(plan):
    q = [free_of_front(2), free_of_front(4, 1)]
    out = plan(TREE, q)
    assert out["levels"] == [[(2, 0b01), (4, 0b10)], [(6, 0b01)], [(7, 0b11)]]
    assert check_one_front_per_level(TREE, q, out) == [[2, 6, 7], [4, 7]]


def test_two_queries_in_one_front_share_it(plan):
    q = [free_of_front(1, 0), free_of_front(1, 1)]
    out = plan(TREE, q)
    assert out["levels"] == [[(1, 0b11)], [(5, 0b11)], [(7, 0b11)]] and out["n_path"] == 3
    check_one_front_per_level(TREE, q, out)


def test_paths_that_merge_carry_both_columns_from_the_merge_upward(plan):
    q = [free_of_front(0), free_of_front(1), free_of_front(3), free_of_front(6)]
    out = plan(TREE, q)
    assert out["levels"] == [[(0, 0b0001), (1, 0b0010), (3, 0b0100)], [(5, 0b0011), (6, 0b1100)], [(7, 0b1111)]]
    check_one_front_per_level(TREE, q, out)


def test_the_gauge_node_is_a_query_without_a_path(plan):
    q = [-1, free_of_front(5)]
    out = plan(TREE, q)
    assert out["levels"] == [[], [(5, 0b10)], [(7, 0b10)]] and out["query_front"] == [-1, 5]
    check_one_front_per_level(TREE, q, out)


def binary_tree(depth, per_front):
    """complete binary tree, fronts numbered level by level from the leaves; front k eliminates per_front consecutive positions"""
    parent, level, first_of_level = [], [], []
    for l in range(depth):
        first_of_level.append(len(parent))
        width = 2 ** (depth - 1 - l)
        for t in range(width):
            level.append(l)
            parent.append(-1 if l == depth - 1 else first_of_level[l] + width + t // 2)
    n = len(parent) * per_front
    # (a fixed shuffle of the free nodes over the elimination positions)
    elim_of_free = [(37 * f + 11) % n for f in range(n)]
    assert sorted(elim_of_free) == list(range(n))
    return parent, level, [e // per_front for e in range(n)], elim_of_free


def test_sixty_four_queries_and_the_limit(plan):
    tree = binary_tree(5, 3)                                   # 31 fronts, 93 free nodes
    q = list(range(64))
    out = plan(tree, q)
    paths = check_one_front_per_level(tree, q, out)
    assert out["front_mask"][30] == 2 ** 64 - 1                # every path ends in the root
    assert all(len(p) == 5 - tree[1][p[0]] for p in paths)
    assert plan(tree, list(range(65))) is None                 # one more than a mask holds
    assert plan(tree, [93]) is None                            # not a free node
    q = [92, 0, 45]
    check_one_front_per_level(tree, q, plan(tree, q))
