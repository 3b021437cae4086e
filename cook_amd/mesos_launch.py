"""The two ends of Engine.match_launch_resources for a Mesos pool (mesos/task.clj:171-293, :404-416): `rows_from_offers` turns the hosts'
Mesos offer maps into the role view the call reads (resources-by-role, column by column), `messages` turns one task's slice of its
result into the reference's :scalar-resource-messages / :ports-resource-messages maps and the PORTn pairs."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from . import _abi as A


def rows_from_offers(hosts: Sequence[Sequence[dict]], roles: Sequence[str], names: Sequence[str] = ("cpus", "mem"),
                     sources: Optional[Dict[str, int]] = None, offer_skipped=None) -> A.LaunchOffers:
    """hosts[v]: the Mesos offers of offer row v of the match, each {"resources": [{"name", "type", "role", "scalar" | "ranges"}, ...]}
    (the maps compile-mesos-messages is given).  roles: the pool's role names in TAKE order, "*" last: the order of
    (sort-by #(= "*" %) (keys avail)).  That order is the key order of each host's own map, so with several roles besides "*" every
    host must list them in this order: a host that does not is refused (ValueError), as is a role that is not in `roles`.  names: the
    resource name of each slot, in getScalarRequests' order; sources: name -> A.LAUNCH_CPUS / A.LAUNCH_MEM / A.LAUNCH_SCALAR0 + s
    (default: "cpus" and "mem").  A role a host does not have: amount 0.0, no range.  The ranges of a row are in the order of its
    offers' "ports" resources ((reduce into))."""
    roles = list(roles)
    if "*" in roles and roles[-1] != "*":
        raise ValueError('the "*" role is taken last')
    if not 1 <= len(roles) <= A.MAX_ROLES:
        raise ValueError("1 .. %d roles" % A.MAX_ROLES)
    src = dict(cpus=A.LAUNCH_CPUS, mem=A.LAUNCH_MEM) if sources is None else sources
    n, n_roles, n_res = len(hosts), len(roles), len(names)
    avail = np.zeros((n_res, n_roles, n))
    seen = np.zeros((n_res, n_roles, n), bool)
    off, begin, end, role_of = [0], [], [], []
    for v, offers in enumerate(hosts):
        order = {}  # resource name -> the roles in the order the host's map lists them (group-by: first appearance)
        for offer in offers:
            for res in offer["resources"]:
                if res["role"] not in roles:
                    raise ValueError("host %d: role %r is not among the pool's roles" % (v, res["role"]))
                x = roles.index(res["role"])
                order.setdefault(res["name"], [])
                if x not in order[res["name"]]:
                    order[res["name"]].append(x)
                if res["name"] == "ports":
                    for rg in res["ranges"]:
                        begin.append(rg["begin"]), end.append(rg["end"]), role_of.append(x)
                elif res["name"] in names and res["type"] == "value-scalar":
                    r = names.index(res["name"])
                    avail[r, x, v] = res["scalar"] if not seen[r, x, v] else avail[r, x, v] + res["scalar"]  # (reduce +), in offer order
                    seen[r, x, v] = True
        for name, xs in order.items():
            rest = [x for x in xs if roles[x] != "*"]
            if name in names and rest != sorted(rest):
                raise ValueError("host %d lists the roles of %r in another order than the pool's take order" % (v, name))
        off.append(len(begin))
    return A.LaunchOffers(n=n, n_roles=n_roles, range_off=np.asarray(off, np.uint32), range_begin=np.asarray(begin, np.int32),
                          range_end=np.asarray(end, np.int32), range_role=np.asarray(role_of, np.uint8),
                          res_source=np.asarray([src[nm] for nm in names], np.uint32), avail=avail,
                          offer_skipped=None if offer_skipped is None else np.asarray(offer_skipped, np.uint8))


def messages(result: dict, k: int, names: Sequence[str], roles: Sequence[str]) -> dict:
    """considered position k of Engine.match_launch_resources' result as the reference decorates a task: scalar_resource_messages (slot
    after slot, role after role in take order; a take of 0.0 is no message), ports_resource_messages (one per assigned port),
    ports_assigned (ascending) and port_env (the PORT0..PORTn variables)."""
    lo, hi = int(result["port_off"][k]), int(result["port_off"][k + 1])
    ports = [int(p) for p in result["port"][lo:hi]]
    scalar = [{"name": names[r], "type": "value-scalar", "role": roles[x], "scalar": float(result["take"][k][r][x])}
              for r in range(len(names)) for x in range(len(roles)) if result["take"][k][r][x] > 0]
    port_msgs = [{"name": "ports", "type": "value-ranges", "role": roles[int(x)], "ranges": [{"begin": p, "end": p}]}
                 for p, x in zip(ports, result["port_role"][lo:hi])]
    return dict(scalar_resource_messages=scalar, ports_resource_messages=port_msgs, ports_assigned=ports,
                port_env={"PORT%d" % i: str(p) for i, p in enumerate(ports)})
