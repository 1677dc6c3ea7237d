# The client of jpeg_read_coefficients (TEST INFRASTRUCTURE, tests/coef_cases.py), built like djpeg_client: against the reference's
# headers, linked to the reference's library; the binary travels to the GPU box with the tree.
#   make -C tests/native -f coef_dump.mk
REF ?= /root/reference
INC = -I../../oracle/_ref/include -I$(REF)
all: coef_dump
coef_dump: coef_dump.c
	gcc -O2 -Wall $(INC) -o $@ $< -L../../oracle/_ref -l:libjpeg.so.62 -lpthread
