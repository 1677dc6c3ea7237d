# The lossless-mode client of the libjpeg API (TEST INFRASTRUCTURE, tests/test_gpu_lossless_client.py), built like the clients of
# ./Makefile: against the reference's headers, linked to the reference's library; the binary travels to the GPU box with the tree.
#   make -C tests/native -f lossless_client.mk
REF ?= /root/reference
INC = -I../../oracle/_ref/include -I$(REF)
lossless_client: lossless_client.c
	gcc -O2 -Wall $(INC) -o $@ $< -L../../oracle/_ref -l:libjpeg.so.62 -lpthread
