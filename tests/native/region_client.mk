# The client of the libjpeg partial-decompression API (TEST INFRASTRUCTURE, tests/region_cases.py), built like the clients of
# ./Makefile: against the reference's headers, linked to the reference's library; the binary travels to the GPU box with the tree.
#   make -C tests/native -f region_client.mk
REF ?= /root/reference
INC = -I../../oracle/_ref/include -I$(REF)
all: region_client
region_client: region_client.c
	gcc -O2 -Wall $(INC) -o $@ $< -L../../oracle/_ref -l:libjpeg.so.62 -lpthread
