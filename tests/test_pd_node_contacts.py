"""CPU tests of the PD node-node contact switch (PIES_FLAG_PD_NODE_CONTACTS): the flag, the tuning name, the contact count and
the C++ drop-in class's member, on host-only handles (PIES_DEVICE_NONE) and without a device."""
import os
import subprocess

import numpy as np

from pies_amd import capi
from test_dropin_cpp import build_example

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "pd_node_contacts_example.cpp")


def host_handle():
    g = capi.Solver(capi.Options(solver=capi.PD, iterations=4), device=capi.DEVICE_NONE)
    g.add_nodes_raw(np.float32([[0, 1, 0], [0.5, 1, 0], [3, 1, 0]]), radius=0.5)
    return g


def test_constants_match_the_header():
    assert capi.FLAG_PD_NODE_CONTACTS == 6
    assert capi.NODE_CONTACTS == 20
    assert "pies_get_node_contacts" in capi.SYMBOLS


def test_host_handle_accepts_flag_and_tuning():
    g = host_handle()
    g.set_flag(capi.FLAG_PD_NODE_CONTACTS, 1)
    capi.set_tuning("PIES_PD_NODE_CONTACT_PARTNERS", 8)
    try:
        g.finalize()
    finally:
        capi.set_tuning("PIES_PD_NODE_CONTACT_PARTNERS", None)
    g.set_flag(capi.FLAG_PD_NODE_CONTACTS, 0)
    g.finalize()


def test_no_contacts_before_a_tick():
    g = host_handle()
    assert g.count(capi.NODE_CONTACTS) == 0
    g.set_flag(capi.FLAG_PD_NODE_CONTACTS, 1)
    g.finalize()
    assert g.count(capi.NODE_CONTACTS) == 0
    assert g.node_contacts().shape == (0, 2)


def test_cpp_member_survives_a_move(tmp_path):
    out = subprocess.run([build_example(tmp_path, SRC)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-400:], out.stderr[-400:])
    assert "move ok" in out.stdout
