"""The packet walk's slot order (pysicalbasedraytracer_amd/csrc/pbr_quad_order.h) compiled for the host
(tests/cpp_quad_order/quad_order_test.cpp), against a direct statement of the documented rule: a quad
node holds the children of binary node N's first child A in columns 0, 1 and of its second child B in
columns 2, 3; the near child of the top split is visited first, and inside each half the near child of
that half's split, near being the second child where the ray's direction is negative on the split axis.
The wave enters the first position some lane passes and pushes the later passing ones far-last.

The program is built twice, plain and with the address and undefined-behaviour sanitizers, and both are
run as programs of their own."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "cpp_quad_order")


def rule(aN, aA, aB, oct_, valid, passing):
    """(visit order as columns, values in visit order, entered position, pushes) by the rule above."""
    def near_first(axis, pair):
        return pair[::-1] if (oct_ >> axis) & 1 else pair
    halves = near_first(aN, [near_first(aA, [0, 1]), near_first(aB, [2, 3])])
    order = halves[0] + halves[1]
    some = valid & passing
    value = [(0x100000001 << c) if (some >> c) & 1 else 0 for c in range(4)]
    m = [value[c] for c in order]
    hit = [pos for pos in range(4) if m[pos]]
    first = hit[0] if hit else -1
    pushes = [(pos, order[pos], m[pos]) for pos in reversed(hit[1:])]
    return order, m, first, pushes


def parse(line):
    key, order, m, first, pushes = line.split("|")
    return (tuple(int(x) for x in key.split()), [int(x) for x in order.split()], [int(x, 16) for x in m.split()], int(first),
            [(int(a), int(b), int(c, 16)) for a, b, c in (p.split(":") for p in pushes.split())])


@pytest.fixture(scope="module")
def programs():
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    return os.path.join(DIR, "quad_order_test"), os.path.join(DIR, "quad_order_test_san")


def run(path):
    p = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stderr == "", p.stderr[-2000:]   # a sanitizer report
    return p.stdout


def test_every_case_follows_the_rule(programs):
    lines = run(programs[0]).splitlines()
    assert len(lines) == 27 * 8 * 16 * 16
    seen = set()
    orders = set()
    for line in lines:
        key, order, m, first, pushes = parse(line)
        seen.add(key)
        assert (order, m, first, pushes) == rule(*key), line
        orders.add(tuple(order))
    assert len(seen) == len(lines)   # every (axes, octant, valid, pass) once
    # the eight orders a quad node can have: each half's pair either way, the halves either way
    assert len(orders) == 8


def test_sanitized_build_prints_the_same(programs):
    assert run(programs[1]) == run(programs[0])
