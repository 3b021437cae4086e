"""Oracle of cook_match_launch_resources: a literal restatement, over dicts, of the reference's mesos/task.clj functions
(resources-by-role, range-contains?, role-containing-port, take-ports, take-resources, take-all-scalar-resources-for-task,
add-scalar-resources-to-task-infos) and of the port-cursor rule of include/cookmatch.h ("LAUNCH RESOURCES": Fenzo's own source is not
in the tree, so that rule is oracle-defined).  Plain Python floats and lists, no numpy: every subtraction is the fp64 operation the
reference's reduce performs, in its order.  It owes nothing to the engine's layout: `launch` works on hosts, tasks and names, and
`as_arrays` (the only function that knows the layout) turns its result into what the engine returns."""
from __future__ import annotations

import math


# ---- mesos/task.clj:171-192 ----------------------------------------------------------------------------------------------------------
def combine_like_resources(resources):
    if resources[0]["type"] == "value-scalar":
        total = resources[0]["scalar"]          # (reduce +): the first value, then left to right
        for r in resources[1:]:
            total = total + r["scalar"]
        return total
    out = []                                    # :value-ranges: (reduce into)
    for r in resources:
        out = out + list(r["ranges"])
    return out


def group_by(key, items):
    out = {}
    for it in items:
        out.setdefault(it[key], []).append(it)
    return out


def resources_by_role(offers):
    flat = [r for o in offers for r in o["resources"]]
    return {name: {role: combine_like_resources(rs) for role, rs in group_by("role", named).items()}
            for name, named in group_by("name", flat).items()}


# ---- :194-221 ------------------------------------------------------------------------------------------------------------------------
def range_contains(val, mesos_range):
    return mesos_range["begin"] <= val and mesos_range["end"] >= val


def role_containing_port(available_ports, port):
    for role, ranges in available_ports.items():
        if any(range_contains(port, r) for r in ranges):
            return role
    return None


def take_ports(available_ports, ports_needed):
    return [{"name": "ports", "type": "value-ranges", "role": role_containing_port(available_ports, p), "ranges": [{"begin": p, "end": p}]}
            for p in ports_needed]


# ---- :238-293 ------------------------------------------------------------------------------------------------------------------------
def take_resources(available_resources, resource_name, amount):
    avail = available_resources.get(resource_name) or {}
    sorted_roles = sorted(avail.keys(), key=lambda role: role == "*")  # (sort-by #(= "*" %)): stable, "*" last
    state = {"amount-still-needed": amount, "mesos-messages": [], "remaining-resources": dict(avail)}
    for role_name in sorted_roles:
        amount_avail = state["remaining-resources"].get(role_name) or 0
        amount_to_take = min(state["amount-still-needed"], amount_avail)
        if amount_to_take > 0:
            remaining = dict(state["remaining-resources"])
            remaining[role_name] = amount_avail - amount_to_take
            state = {"amount-still-needed": state["amount-still-needed"] - amount_to_take,
                     "mesos-messages": state["mesos-messages"] + [{"name": resource_name, "role": role_name, "scalar": amount_to_take, "type": "value-scalar"}],
                     "remaining-resources": remaining}
    return state


def take_all_scalar_resources_for_task(resources, scalar_requests, still_needed=None):
    """scalar_requests: getScalarRequests, {name: amount} in its order.  still_needed (optional dict): filled with each name's
    :amount-still-needed, which the reference computes and drops"""
    state = {"mesos-messages": [], "remaining-resources": resources}
    for resource_name, amount in scalar_requests.items():
        adjustment = take_resources(state["remaining-resources"], resource_name, amount)
        remaining = dict(state["remaining-resources"])
        remaining[resource_name] = adjustment["remaining-resources"]
        state = {"mesos-messages": state["mesos-messages"] + adjustment["mesos-messages"], "remaining-resources": remaining}
        if still_needed is not None:
            still_needed[resource_name] = adjustment["amount-still-needed"]
    return state


def add_scalar_resources_to_task_infos(available_resources, tasks):
    """tasks: dicts with "scalar-requests"; -> the tasks with :scalar-resource-messages (and "still-needed" beside them)"""
    handled, remaining = [], available_resources
    for task in tasks:
        still = {}
        adjustment = take_all_scalar_resources_for_task(remaining, task["scalar-requests"], still)
        handled.append(dict(task, **{"scalar-resource-messages": adjustment["mesos-messages"], "still-needed": still}))
        remaining = adjustment["remaining-resources"]
    return handled


def add_ports_to_task_info(available_resources, tasks):
    available_ports = available_resources.get("ports") or {}
    out = []
    for task in tasks:
        ports = task["ports-assigned"]
        out.append(dict(task, **{"ports-resource-messages": take_ports(available_ports, ports),
                                 "port-env": {"PORT%d" % i: str(p) for i, p in enumerate(ports)}}))
    return out


# ---- the port-cursor rule --------------------------------------------------------------------------------------------------------------
def assign_ports(lease_ranges, counts):
    """lease_ranges: the host's ranges in lease order; counts: the ports each task asks for, in assignment order.  A fresh set of
    leases starts the cursor at 0; the c-th consumed port is the c-th port of the ranges concatenated in their order; each task's
    ports come back sorted ((vec (sort getAssignedPorts))).  -> a list of lists, or None when the ranges do not hold them all"""
    cursor, out = 0, []
    held = sum(r["end"] - r["begin"] + 1 for r in lease_ranges)
    for n in counts:
        if cursor + n > held:
            return None
        mine = []
        for c in range(cursor, cursor + n):
            left = c
            for r in lease_ranges:
                size = r["end"] - r["begin"] + 1
                if left < size:
                    mine.append(r["begin"] + left)
                    break
                left -= size
        cursor += n
        out.append(sorted(mine))
    return out


def host_fault(host):
    """what cook_match_launch_resources refuses a row for, whatever its tasks: ranges not 0 <= begin <= end or not pairwise disjoint, an
    amount that is not finite and >= 0"""
    rs = host["lease-ranges"]
    for i, r in enumerate(rs):
        if r["begin"] < 0 or r["begin"] > r["end"]:
            return True
        if any(r["begin"] <= q["end"] and q["begin"] <= r["end"] for q in rs[:i]):
            return True
    for name, by_role in host["resources"].items():
        if name != "ports" and any(not (math.isfinite(a) and a >= 0) for a in by_role.values()):
            return True
    return False


def launch(hosts, tasks, skipped=None):
    """hosts[v] = {"resources": resources-by-role's map (with "ports"), "lease-ranges": the host's ranges in lease order};
    tasks[k] (considered order) = {"offer": v or -1, "ports": count, "scalar-requests": {name: amount}}; skipped[v] truthy: the offer's
    tasks are not launched.  -> (per task: None when not kept, else the decorated task: "ports-assigned", "ports-resource-messages",
    "scalar-resource-messages", "still-needed"; bad_row: the lowest row that is refused, or None)"""
    out = [None] * len(tasks)
    bad = None
    on_offer = {}
    for k, t in enumerate(tasks):
        on_offer.setdefault(t["offer"], []).append(k)
    for v, host in enumerate(hosts):
        mine = [] if (skipped is not None and skipped[v]) else on_offer.get(v, [])
        ports = assign_ports(host["lease-ranges"], [tasks[k]["ports"] for k in mine])
        if host_fault(host) or ports is None:
            bad = v if bad is None else bad
            continue
        infos = [dict(tasks[k], **{"ports-assigned": p}) for k, p in zip(mine, ports)]
        infos = add_scalar_resources_to_task_infos(host["resources"], infos)
        infos = add_ports_to_task_info(host["resources"], infos)
        for k, info in zip(mine, infos):
            out[k] = info
    return out, bad


# ---- the engine's arrays -----------------------------------------------------------------------------------------------------------------
def as_arrays(result, names, roles):
    """launch's result as cook_match_launch_resources returns it: port_off, port, port_role, take[k][r][role] (floats; 0.0 = no
    message), short_mask, and the counts of cook_launch_info"""
    port_off, port, port_role, take, short = [0], [], [], [], []
    for info in result:
        row = [[0.0] * len(roles) for _ in names]
        mask = 0
        if info is not None:
            for m in info["ports-resource-messages"]:
                port.append(m["ranges"][0]["begin"])
                port_role.append(roles.index(m["role"]))
            for m in info["scalar-resource-messages"]:
                row[names.index(m["name"])][roles.index(m["role"])] = m["scalar"]
            for name, left in info["still-needed"].items():
                if left != 0:
                    mask |= 1 << names.index(name)
        port_off.append(len(port))
        take.append(row)
        short.append(mask)
    kept = [i for i in result if i is not None]
    return dict(port_off=port_off, port=port, port_role=port_role, take=take, short_mask=short,
                info=dict(kept=len(kept), ports=len(port), offers_used=len({i["offer"] for i in kept}), short_tasks=sum(1 for m in short if m)))
