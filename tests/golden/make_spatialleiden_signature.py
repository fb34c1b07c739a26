"""Extracts the signature of the reference's ``calculate_niche_spatialleiden`` (AST only; nothing is imported or executed) into
tests/golden/spatialleiden_signature.json: parameter names in positional order and their defaults as Python source.

    python tests/golden/make_spatialleiden_signature.py <root of the reference checkout>"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FILE, NAME = "src/squidpy/gr/_niche.py", "calculate_niche_spatialleiden"

with open(os.path.join(sys.argv[1], FILE)) as fh:
    tree = ast.parse(fh.read())
node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == NAME)
a = node.args
names = [x.arg for x in a.args]
defaults = [None] * (len(names) - len(a.defaults)) + [ast.unparse(d) for d in a.defaults]
out = {"function": NAME, "file": f"{FILE}:{node.lineno}", "positional": [{"name": n, "default": d} for n, d in zip(names, defaults)],
       "keyword_only": [{"name": k.arg, "default": ast.unparse(d) if d is not None else None} for k, d in zip(a.kwonlyargs, a.kw_defaults)]}
with open(os.path.join(HERE, "spatialleiden_signature.json"), "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(out)
