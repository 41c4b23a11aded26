#!/usr/bin/env python
"""Golden fixture of the reference's public call surface (authoring side only; needs a read-only reference checkout).

    python tests/golden/make_golden_api.py REFERENCE_CHECKOUT

Writes tests/golden/reference_api.json: the parameter names and defaults of the five operators of
`model.stylegan.op` and of its CPU twin `model.stylegan.op_cpu`, the option table (dest -> kind, default) of
style_transfer.py, and the options of the RAFT argument parser in smooth_parsing_map.py.  The sources are parsed
(ast), never imported or executed, and only names and literal values are stored: the tests compare this
repository's operator surface, command line and RAFT construction against it without the reference present."""
import ast
import json
import os
import sys

OPS = {"upfirdn2d": ("upfirdn2d.py", "upfirdn2d"), "fused_leaky_relu": ("fused_act.py", "fused_leaky_relu"),
       "FusedLeakyReLU.__init__": ("fused_act.py", "FusedLeakyReLU.__init__"),
       "conv2d_gradfix.conv2d": ("conv2d_gradfix.py", "conv2d"),
       "conv2d_gradfix.conv_transpose2d": ("conv2d_gradfix.py", "conv_transpose2d")}


def _value(node):
    """A default's value: literals, and constant arithmetic such as 2 ** 0.5."""
    return eval(compile(ast.Expression(node), "<default>", "eval"), {"__builtins__": {}})


def _find(tree, dotted):
    nodes = tree.body
    for part in dotted.split("."):
        node = next(n for n in nodes if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name == part)
        nodes = node.body
    return node


def signature(path, dotted):
    fn = _find(ast.parse(open(path).read()), dotted)
    names = [a.arg for a in fn.args.args]
    defaults = dict(zip(names[len(names) - len(fn.args.defaults):], (_value(d) for d in fn.args.defaults)))
    return {"params": names, "defaults": defaults}


def options(path, receiver):
    """dest -> [kind, default] of every add_argument call on `receiver` ("self.parser" or "parser")."""
    out = {}
    for node in ast.walk(ast.parse(open(path).read())):
        if not (isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument"):
            continue
        if ast.unparse(node.func.value) != receiver:
            continue
        kw = {k.arg: k.value for k in node.keywords}
        dest = node.args[0].value.lstrip("-")
        if "action" in kw:
            out[dest] = [kw["action"].value, False]
        else:
            out[dest] = [kw["type"].id if "type" in kw else None, _value(kw["default"]) if "default" in kw else None]
    return out


def main(ref):
    op_dir = os.path.join(ref, "model", "stylegan")
    api = {pkg: {name: signature(os.path.join(op_dir, pkg, f), d) for name, (f, d) in OPS.items()}
           for pkg in ("op", "op_cpu")}
    api["style_transfer_options"] = options(os.path.join(ref, "style_transfer.py"), "self.parser")
    api["raft_options"] = options(os.path.join(ref, "smooth_parsing_map.py"), "parser")
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_api.json")
    with open(out, "w") as f:
        json.dump(api, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out)


if __name__ == "__main__":
    main(sys.argv[1])
