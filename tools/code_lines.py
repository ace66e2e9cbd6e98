"""Raw lines and code lines of Python files: a code line holds a token that is neither a comment nor part of a docstring (blank lines,
comment-only lines and docstrings are not counted).      python tools/code_lines.py FILE..."""
import ast
import io
import sys
import tokenize

SKIP = (tokenize.COMMENT, tokenize.NL, tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT, tokenize.ENDMARKER)
total = [0, 0]
for path in sys.argv[1:]:
    src = open(path).read()
    doc = set()
    for n in ast.walk(ast.parse(src)):
        if isinstance(n, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and ast.get_docstring(n, clean=False) is not None:
            doc.update(range(n.body[0].lineno, n.body[0].end_lineno + 1))
    code = set()
    for t in tokenize.generate_tokens(io.StringIO(src).readline):
        if t.type not in SKIP:
            code.update(range(t.start[0], t.end[0] + 1))
    raw, n = src.count("\n"), len(code - doc)
    total = [total[0] + raw, total[1] + n]
    print(f"{path}: {raw} lines, {n} code lines")
print(f"total: {total[0]} lines, {total[1]} code lines")
