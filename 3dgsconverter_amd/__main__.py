"""``python -m 3dgsconverter_amd``: the command line (cli.py)"""
from .cli import main

main()
